// airfe — the order in which the persistent 3x3 convolution kernels (kernels_conv64r.hip, kernels_conv128r.hip) walk
// their tiles, stated once for both kernels, their launchers and the host check (tools/conv_tile_order_check.cpp).
// Integer arithmetic only; usable from host and device.
//
// Workgroup b of a launch runs on XCD b % 8 (the placement every streaming kernel of this library relies on for L2
// reuse; a wrong guess is slower, never wrong).  Two walks:
//   * RASTER (order 0, and every grid that is no multiple of 8): workgroup b takes tile b + i * grid in iteration i,
//     tiles in row-major order image by image; a layer with more output channels than one pass holds is one launch
//     per pass.
//   * BLOCKED: with per_xcd = grid / 8, x = b & 7 and s = b >> 3 the workgroup takes work item
//     n = (i * 8 + x) * per_xcd + s.  The pass is s % passes, so the `passes` workgroups that read one input tile sit
//     on one XCD in one iteration and the layer is ONE launch; the tile is item (i * 8 + x) * chunk + s / passes
//     (chunk = per_xcd / passes) of a blocked order of the tile grid: bw x bh-tile blocks row-major inside an image,
//     tiles row-major inside a block, bw * bh = chunk where the image allows it — the tiles an XCD holds in one
//     iteration are one compact 2-D block of one image (or whole images), and their halos meet in that XCD's L2.
// The raster order is the blocked order with bw = tiles_x, bh = 1: one decode serves both.
#pragma once

#if defined(__HIPCC__)
#define AIRFE_CTO_FN __host__ __device__ __forceinline__
#else
#define AIRFE_CTO_FN inline
#endif

namespace airfe {

constexpr int CONV_XCDS = 8;

struct ConvTileOrder {
  int tiles_x = 0, per_img = 0, ntiles = 0;   // tiles per row, per image, in the batch
  int passes = 1, sh_pass = 0;                // cout passes walked inside the launch (a power of two), its log2
  int pass0 = 0;                              // the launch's first pass (the raster walk launches once per pass)
  int chunk = 0;                              // tiles an XCD takes per iteration; 0: raster walk
  // power-of-two tile grids (every size of this network): shifts.  Otherwise -1: two divisions, raster order
  int sh_img = -1, sh_x = -1;                 // log2 per_img, log2 tiles_x
  int sh_bw = 0, sh_blk = 0;                  // log2 bw, log2 (bw * bh)
};

AIRFE_CTO_FN bool conv_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
AIRFE_CTO_FN int conv_log2(int v) {
  int s = 0;
  while ((1 << (s + 1)) <= v) ++s;
  return s;
}

// The plan of one launch.  order 0: raster.  tile_w x tile_h: the tile in pixels (the block is grown toward a square of pixels).
// Blocked needs grid % 8 == 0 and passes a power of two that divides grid / 8; everything else keeps the raster walk,
// one launch per pass (the caller loops pass0 over `conv_tile_launches`).
AIRFE_CTO_FN ConvTileOrder conv_tile_order(int order, int grid, int tiles_x, int tiles_y, int images, int passes, int tile_w, int tile_h) {
  ConvTileOrder o;
  o.tiles_x = tiles_x;
  o.per_img = tiles_x * tiles_y;
  o.ntiles = o.per_img * images;
  const bool p2 = conv_pow2(tiles_x) && conv_pow2(tiles_y);
  if (p2) {
    o.sh_x = conv_log2(tiles_x);
    o.sh_img = conv_log2(o.per_img);
    o.sh_bw = o.sh_x;                         // bw = tiles_x, bh = 1: raster
    o.sh_blk = o.sh_x;
  }
  const int per_xcd = grid / CONV_XCDS;
  if (!order || grid < CONV_XCDS || grid % CONV_XCDS || !conv_pow2(passes) || per_xcd % passes) return o;
  o.passes = passes;
  o.sh_pass = conv_log2(passes);
  o.chunk = per_xcd / passes;
  if (p2) {
    int bw = 1, bh = 1;
    while (bw * bh * 2 <= o.chunk) {
      const bool gx = bw * 2 <= tiles_x, gy = bh * 2 <= tiles_y;
      if (gx && (bw * tile_w <= bh * tile_h || !gy)) bw *= 2;
      else if (gy) bh *= 2;
      else break;                             // the block is the whole image: an XCD takes whole images
    }
    o.sh_bw = conv_log2(bw);
    o.sh_blk = conv_log2(bw * bh);
  }
  return o;
}
// the launches a layer of `passes` cout passes takes under plan o (the caller steps o.pass0 through them)
AIRFE_CTO_FN int conv_tile_launches(const ConvTileOrder& o, int passes) { return o.chunk ? 1 : passes; }

// workgroup wg of `grid`: its first tile item, the step from one iteration to the next, and its pass.  The walk is
//   for (tile = first; tile < o.ntiles; tile += step)
AIRFE_CTO_FN void conv_tile_first(const ConvTileOrder& o, int wg, int grid, int& first, int& step, int& pass) {
  if (o.chunk) {
    const int x = wg & (CONV_XCDS - 1), s = wg >> 3;
    first = x * o.chunk + (s >> o.sh_pass);
    step = CONV_XCDS * o.chunk;
    pass = o.pass0 + (s & (o.passes - 1));
  } else {
    first = wg;
    step = grid;
    pass = o.pass0;
  }
}

// tile item -> (image, tile row, tile column).  Two forms, chosen by the plan (sh_img >= 0: shifts): a kernel at its register limit compiles one
// instantiation per form (conv128r_kernel), the others branch (wave-uniform)
AIRFE_CTO_FN void conv_tile_decode_shift(const ConvTileOrder& o, int tile, int& b, int& ty, int& tx) {
  b = tile >> o.sh_img;
  const int rem = tile & (o.per_img - 1);
  const int blk = rem >> o.sh_blk, w = rem & ((1 << o.sh_blk) - 1);
  const int sh_bx = o.sh_x - o.sh_bw, sh_bh = o.sh_blk - o.sh_bw;
  ty = ((blk >> sh_bx) << sh_bh) + (w >> o.sh_bw);
  tx = ((blk & ((1 << sh_bx) - 1)) << o.sh_bw) + (w & ((1 << o.sh_bw) - 1));
}
AIRFE_CTO_FN void conv_tile_decode_div(const ConvTileOrder& o, int tile, int& b, int& ty, int& tx) {
  b = tile / o.per_img;
  const int rem = tile - b * o.per_img;
  ty = rem / o.tiles_x;
  tx = rem - ty * o.tiles_x;
}
AIRFE_CTO_FN void conv_tile_decode(const ConvTileOrder& o, int tile, int& b, int& ty, int& tx) {
  if (o.sh_img >= 0) conv_tile_decode_shift(o, tile, b, ty, tx);
  else conv_tile_decode_div(o, tile, b, ty, tx);
}

// (workgroup, iteration) -> (pass, image, tile row, tile column); false: the workgroup has no tile in that iteration
AIRFE_CTO_FN bool conv_tile_map(const ConvTileOrder& o, int wg, int i, int grid, int& pass, int& b, int& ty, int& tx) {
  int first, step;
  conv_tile_first(o, wg, grid, first, step, pass);
  const long long tile = (long long)first + (long long)i * step;
  if (tile >= o.ntiles) return false;
  conv_tile_decode(o, (int)tile, b, ty, tx);
  return true;
}

}  // namespace airfe
