// Host check of csrc/conv_tile_order.h: enumerates the (workgroup, iteration) -> (pass, image, tile row, tile column) map of the persistent conv kernels
// for both orders and asserts what the kernels rely on.  Stand-alone (tests/test_conv_tile_order_cpu.py builds it with the address and undefined-behaviour
// sanitizers and runs it); prints one line per case, exit status 1 on the first violated property.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -Iairslam_amd/csrc tools/conv_tile_order_check.cpp -o conv_tile_order_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv_tile_order.h"

using namespace airfe;

struct Case {
  const char* name;
  int kernel;            // 64: conv64r (16 x 16-pixel tiles), 128: conv128r (16 wide x 8 high)
  int B, H, W, passes, wgs;
  bool bench;            // a benchmark shape: the blocked order's compactness and halo share are asserted, not only printed
};

struct Visit { int count = 0, label = -1, iter = -1, launch = -1; };

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAIL %s order %d: ", c.name, order);    \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
      g_fail = 1;                                          \
      return -1.0;                                         \
    }                                                      \
  } while (0)

// walks one layer as its launcher does; returns the share of (lower, right) neighbour pairs of a tile that run on the same XCD label in the same iteration
static double run(const Case& c, int order) {
  const int tw = 16, th = c.kernel == 64 ? 16 : 8;
  const int tiles_x = c.W / tw, tiles_y = c.H / th, per_img = tiles_x * tiles_y, ntiles = per_img * c.B;
  const int grid = ntiles < c.wgs ? ntiles : c.wgs;
  ConvTileOrder o = conv_tile_order(order, grid, tiles_x, tiles_y, c.B, c.passes, tw, th);
  const int launches = conv_tile_launches(o, c.passes);
  CHECK(launches == 1 || launches == c.passes, "%d launches", launches);
  const bool blocked = o.chunk != 0;
  CHECK(blocked == (order && grid >= 8 && grid % 8 == 0 && conv_pow2(c.passes) && (grid / 8) % c.passes == 0), "blocked = %d at grid %d, passes %d", (int)blocked, grid, c.passes);
  std::vector<Visit> seen((size_t)c.passes * ntiles);
  for (; o.pass0 < launches; ++o.pass0) {
    int lo = 1 << 30, hi = 0;
    for (int wg = 0; wg < grid; ++wg) {
      int n = 0;
      for (int i = 0;; ++i) {
        int pass, b, ty, tx;
        if (!conv_tile_map(o, wg, i, grid, pass, b, ty, tx)) {
          int p2, b2, y2, x2;                                              // the walk ends for good: no tile in any later iteration
          CHECK(!conv_tile_map(o, wg, i + 1, grid, p2, b2, y2, x2), "workgroup %d has a tile after an empty iteration %d", wg, i);
          break;
        }
        CHECK(pass >= 0 && pass < c.passes && b >= 0 && b < c.B && ty >= 0 && ty < tiles_y && tx >= 0 && tx < tiles_x,
              "workgroup %d iteration %d -> pass %d image %d tile (%d, %d) out of range", wg, i, pass, b, ty, tx);
        if (!blocked) {                                                    // today's order, stated independently: tile wg + i * grid, row-major, pass = the launch
          const int t = wg + i * grid;
          CHECK(pass == o.pass0 && b == t / per_img && ty == t % per_img / tiles_x && tx == t % tiles_x, "raster walk: workgroup %d iteration %d", wg, i);
        }
        Visit& v = seen[((size_t)pass * c.B + b) * per_img + ty * tiles_x + tx];
        ++v.count;
        v.label = wg & 7;
        v.iter = i;
        v.launch = o.pass0;
        ++n;
      }
      lo = n < lo ? n : lo;
      hi = n > hi ? n : hi;
    }
    CHECK(hi - lo <= 1, "tiles per workgroup between %d and %d", lo, hi);
  }
  for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k].count == 1, "(pass, tile) %zu produced %d times", k, seen[k].count);
  auto at = [&](int pass, int b, int ty, int tx) -> const Visit& { return seen[((size_t)pass * c.B + b) * per_img + ty * tiles_x + tx]; };
  if (blocked)
    for (int pass = 1; pass < c.passes; ++pass)
      for (int b = 0; b < c.B; ++b)
        for (int t = 0; t < per_img; ++t) {
          const Visit &p = at(pass, b, t / tiles_x, t % tiles_x), &q = at(0, b, t / tiles_x, t % tiles_x);
          CHECK(p.label == q.label && p.iter == q.iter && p.launch == q.launch, "passes 0 and %d of image %d tile %d: XCD %d / %d, iteration %d / %d", pass, b, t,
                q.label, p.label, q.iter, p.iter);
        }
  long pairs = 0, same = 0;
  for (int b = 0; b < c.B; ++b)
    for (int ty = 0; ty < tiles_y; ++ty)
      for (int tx = 0; tx < tiles_x; ++tx) {
        const Visit& v = at(0, b, ty, tx);
        if (ty + 1 < tiles_y) { const Visit& w = at(0, b, ty + 1, tx); ++pairs; same += w.label == v.label && w.iter == v.iter; }
        if (tx + 1 < tiles_x) { const Visit& w = at(0, b, ty, tx + 1); ++pairs; same += w.label == v.label && w.iter == v.iter; }
      }
  // the tiles one XCD holds in one iteration: one full rectangle of one image, or whole images
  if (blocked && c.bench && ntiles % (8 * o.chunk) == 0) {
    struct Box { int b0 = 1 << 30, b1 = -1, y0 = 1 << 30, y1 = -1, x0 = 1 << 30, x1 = -1, n = 0; };
    std::vector<Box> boxes((size_t)ntiles / o.chunk);                      // one per (iteration, XCD)
    for (int b = 0; b < c.B; ++b)
      for (int t = 0; t < per_img; ++t) {
        const int ty = t / tiles_x, tx = t % tiles_x;
        const Visit& v = at(0, b, ty, tx);
        Box& k = boxes[(size_t)v.iter * 8 + v.label];
        k.b0 = b < k.b0 ? b : k.b0; k.b1 = b > k.b1 ? b : k.b1; k.y0 = ty < k.y0 ? ty : k.y0; k.y1 = ty > k.y1 ? ty : k.y1;
        k.x0 = tx < k.x0 ? tx : k.x0; k.x1 = tx > k.x1 ? tx : k.x1;
        ++k.n;
      }
    for (size_t q = 0; q < boxes.size(); ++q) {
      const Box& k = boxes[q];
      const int i = (int)(q / 8), x = (int)(q % 8);
      CHECK(k.n == o.chunk, "XCD %d iteration %d holds %d tiles, not %d", x, i, k.n, o.chunk);
      if (o.chunk <= per_img) {
        const int bw = k.x1 - k.x0 + 1, bh = k.y1 - k.y0 + 1;
        CHECK(k.b0 == k.b1 && bw * bh == k.n, "XCD %d iteration %d: %d tiles of images %d .. %d in a %d x %d box", x, i, k.n, k.b0, k.b1, bw, bh);
        CHECK(bw * tw <= 2 * bh * th && bh * th <= 2 * bw * tw, "XCD %d iteration %d: a %d x %d-pixel block is not compact", x, i, bw * tw, bh * th);
      } else {
        CHECK((k.b1 - k.b0 + 1) * per_img == k.n, "XCD %d iteration %d: %d tiles over images %d .. %d", x, i, k.n, k.b0, k.b1);
      }
    }
  }
  return pairs ? (double)same / pairs : 1.0;
}

int main() {
  const Case cases[] = {
      // the benchmark's encoder at 128 images, 256 workgroups
      {"conv1 fused 512x512", 64, 128, 512, 512, 1, 256, true},
      {"conv2a/2b 256x256", 64, 128, 256, 256, 1, 256, true},
      {"conv3a 128x128 64->128", 64, 128, 128, 128, 2, 256, true},
      {"conv3b/line 128x128", 128, 128, 128, 128, 1, 256, true},
      {"conv4a/4b 64x64", 128, 128, 64, 64, 1, 256, true},
      {"convPa/Da 64x64 128->256", 128, 128, 64, 64, 2, 256, true},
      {"convPa+Da 64x64, four banks", 128, 128, 64, 64, 4, 256, true},
      // small shapes: wrapped loops, partial last iterations, the fallback grids, a tile grid that is no power of two
      {"conv128r B3 16x32 wgs8", 128, 3, 16, 32, 1, 8, false},
      {"conv128r B3 16x32 wgs16", 128, 3, 16, 32, 1, 16, false},
      {"conv64r B3 16x32 wgs8", 64, 3, 16, 32, 1, 8, false},
      {"conv64r B3 16x32 wgs16", 64, 3, 16, 32, 2, 16, false},
      {"conv128r B5 64x64 wgs8", 128, 5, 64, 64, 1, 8, false},
      {"conv128r B5 64x64 wgs8 p2", 128, 5, 64, 64, 2, 8, false},
      {"conv128r B5 64x64 wgs16 p2", 128, 5, 64, 64, 2, 16, false},
      {"conv128r B5 64x64 wgs64 p2", 128, 5, 64, 64, 2, 64, false},
      {"conv128r B5 64x64 wgs64 p4", 128, 5, 64, 64, 4, 64, false},
      {"conv128r B5 64x64 wgs12", 128, 5, 64, 64, 1, 12, false},
      {"conv128r B5 64x64 wgs12 p2", 128, 5, 64, 64, 2, 12, false},
      {"conv64r B5 64x64 wgs8", 64, 5, 64, 64, 1, 8, false},
      {"conv64r B5 64x64 wgs16 p2", 64, 5, 64, 64, 2, 16, false},
      {"conv64r B5 64x64 wgs64 p4", 64, 5, 64, 64, 4, 64, false},
      {"conv64r B5 64x64 wgs12 p2", 64, 5, 64, 64, 2, 12, false},
      {"conv64r B3 32x48 wgs8", 64, 3, 32, 48, 1, 8, false},
      {"conv64r B3 32x48 wgs16", 64, 3, 32, 48, 1, 16, false},
      {"conv64r B3 32x48 wgs16 p2", 64, 3, 32, 48, 2, 16, false},
      {"conv128r B3 32x48 wgs16 p2", 128, 3, 32, 48, 2, 16, false},
      {"conv128r B3 32x48 wgs24 p3", 128, 3, 32, 48, 3, 24, false},
      {"conv64r B2 64x64 wgs16 p2", 64, 2, 64, 64, 2, 16, false},
      {"conv64r B2 32x32 wgs8", 64, 2, 32, 32, 1, 8, false},
  };
  for (const Case& c : cases) {
    const double raster = run(c, 0), blocked = run(c, 1);
    if (raster < 0 || blocked < 0) return 1;
    std::printf("%-32s passes %d: halo neighbours on the same XCD in the same iteration: raster %.4f, blocked %.4f\n", c.name, c.passes, raster, blocked);
    const int order = 1;
    if (c.bench) {
      if (!(blocked >= raster)) { std::printf("FAIL %s order %d: the blocked share is below the raster order's\n", c.name, order); return 1; }
      // one pass at 64 x 64: an XCD holds whole images, every halo is local.  (Two passes: 16 tiles = half an image, 48 of its 52 pairs.)
      if (c.H == 64 && c.passes == 1 && blocked != 1.0) { std::printf("FAIL %s order %d: share %.4f, expected 1\n", c.name, order, blocked); return 1; }
    }
  }
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
