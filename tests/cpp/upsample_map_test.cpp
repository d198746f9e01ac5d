// upsample_map_test: the HIP-free coordinate arithmetic of the guided upsample
// (epq_raytracer_amd/csrc/hrt_upsample_map.h) as a stand-alone program, for tests/test_upsample_ref.py, which
// compares every word with the numpy restatement (tests/upsample_ref.py), and for a build under ASan + UBSan.
//
// usage: upsample_map_test N [ws wt]...   -- every pair (ws, wt) in 1..N x 1..N, then the listed pairs, each with
// both footprints.  Output (binary, stdout), per footprint, pair and x < wt, eleven 32-bit words:
//   bits(u), bits(x0), nearest, then per tap offset (four slots, ascending; footprint 2 fills two): inside, bits(w).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hrt_upsample_map.h"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

static void emit(std::vector<uint32_t>& out, int footprint, uint32_t ws, uint32_t wt) {
  const float inv_r = hrt::upsample_inv_r(footprint);
  for (uint32_t x = 0; x < wt; ++x) {
    const float u = hrt::upsample_coord(x, ws, wt);
    const float x0 = hrt::upsample_first(u);
    uint32_t rec[11] = {bits(u), bits(x0), hrt::upsample_nearest(x, ws, wt)};
    int slot = 0;
    for (int e = hrt::upsample_tap_lo(footprint); e <= hrt::upsample_tap_hi(footprint); ++e, ++slot) {
      const float xj = x0 + (float)e;
      rec[3 + 2 * slot] = hrt::upsample_inside(xj, ws) ? 1u : 0u;
      rec[4 + 2 * slot] = bits(hrt::upsample_weight(u, xj, inv_r));
    }
    out.insert(out.end(), rec, rec + 11);
  }
}

int main(int argc, char** argv) {
  if (argc < 2 || argc % 2 != 0) {
    std::fprintf(stderr, "usage: %s N [ws wt]...\n", argv[0]);
    return 2;
  }
  const uint32_t n = (uint32_t)std::strtoul(argv[1], nullptr, 10);
  std::vector<uint32_t> out;
  for (int footprint : {2, 4}) {
    for (uint32_t ws = 1; ws <= n; ++ws)
      for (uint32_t wt = 1; wt <= n; ++wt) emit(out, footprint, ws, wt);
    for (int a = 2; a + 1 < argc; a += 2) {
      const uint32_t ws = (uint32_t)std::strtoul(argv[a], nullptr, 10), wt = (uint32_t)std::strtoul(argv[a + 1], nullptr, 10);
      if (ws == 0 || wt == 0 || wt > 16384u) return 2;
      emit(out, footprint, ws, wt);
    }
  }
  return std::fwrite(out.data(), 4, out.size(), stdout) == out.size() ? 0 : 1;
}
