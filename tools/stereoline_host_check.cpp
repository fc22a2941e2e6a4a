// stereoline_host (airslam_amd/csrc/stereoline_core.h) over a few frames written out by hand, as a stand-alone program for a sanitizer build:
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iairslam_amd/csrc tools/stereoline_host_check.cpp \
//       -o stereoline_host_check && ./stereoline_host_check
// Every buffer is sized exactly (no slack), so a read or write past an end is the sanitizer's to find.  Exit status 0 = every status and count as
// written out below (the numbers are those of tests/stereoline_ref.py's hand cases).
#include <stdio.h>

#include <vector>

#include "stereoline_core.h"

static int fails = 0;
static void expect(bool ok, const char* what) {
  if (!ok) { printf("FAIL %s\n", what); ++fails; }
}

int main() {
  const double cam[8] = {2, 60, 3, 40, 512, 512, 320, 240};
  const double T0[16] = {0, -1, 0, 1, 1, 0, 0, 2, 0, 0, 1, 3, 0, 0, 0, 1};
  {  // three left lines, two right lines: a map line, a left line with |dy| = 3, a match equal to the right count
    std::vector<double> left = {352, 240, 352, 496, 100, 100, 100, 103, 352, 100, 352, 200};
    std::vector<double> right = {312, 100, 312, 200, 350, 240, 350, 496};
    std::vector<int32_t> m = {1, 1, 2};
    std::vector<double> sel(12), e(18), p(18);
    std::vector<uint8_t> f(3);
    std::vector<int32_t> st(3);
    int32_t cnt[3];
    stereoline_host(cam, left.data(), 3, right.data(), 2, m.data(), T0, sel.data(), f.data(), st.data(), e.data(), p.data(), cnt);
    expect(st[0] == SL_OK && st[1] == SL_LEFT_HORIZONTAL && st[2] == SL_NO_RIGHT, "statuses");
    expect(cnt[0] == 2 && cnt[1] == 1 && cnt[2] == 1, "counts");
    expect(e[0] == 1.0 && e[1] == 3.25 && e[2] == 23.0 && e[3] == -9.0 && e[4] == 3.25 && e[5] == 23.0, "endpoints worked out on paper");
    expect(p[0] == 0.0 && p[1] == -23.0 && p[2] == 3.25 && p[3] == -1.0 && p[4] == 0.0 && p[5] == 0.0, "Pluecker line worked out on paper");
    expect(f[0] == 1 && f[1] == 1 && f[2] == 0 && sel[8] == 0.0 && sel[4] == 350.0, "selection");
  }
  {  // no lines at all: nothing but the counts is touched (every other pointer is null)
    int32_t cnt[3] = {-7, -7, -7};
    stereoline_host(cam, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, cnt);
    expect(cnt[0] == 0 && cnt[1] == 0 && cnt[2] == 0, "empty frame");
  }
  {  // hostile match indices with ONE right line: nothing is read through them
    std::vector<double> left(16, 100.0), right = {312, 100, 312, 200};
    std::vector<int32_t> m = {2147483647, -2147483647 - 1, 0, 1};
    std::vector<double> sel(16), e(24), p(24);
    std::vector<uint8_t> f(4);
    std::vector<int32_t> st(4);
    int32_t cnt[3];
    stereoline_host(cam, left.data(), 4, right.data(), 1, m.data(), nullptr, sel.data(), f.data(), st.data(), e.data(), p.data(), cnt);
    expect(st[0] == SL_NO_RIGHT && st[1] == SL_NO_RIGHT && st[2] == SL_NO_RIGHT && st[3] == SL_NO_RIGHT && cnt[0] == 0, "hostile indices");
  }
  printf(fails ? "stereoline_host_check: %d failure(s)\n" : "stereoline_host_check: ok\n", fails);
  return fails ? 1 : 0;
}
