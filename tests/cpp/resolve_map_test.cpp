// resolve_map_test: the HIP-free coordinate arithmetic of the fold across resolutions and of hrt_history_phase
// (epq_raytracer_amd/csrc/hrt_resolve_map.h) as a stand-alone program, for tests/test_resolve_ref.py, which compares
// every word with the numpy restatement (tests/resolve_ref.py), and for a build under ASan + UBSan.
//
// usage: resolve_map_test N [ws wt]...   -- every pair (ws, wt) in 1..N x 1..N, then the listed pairs.
// Output (binary, stdout), per pair: nx = resolve_phases(ws, wt), then bits(resolve_phase_offset(a, nx)) for a < nx;
// then for each offset of {-0.5, -0.25, 0, 0.25, 0.5, the nx phase offsets} and each x < wt six 32-bit words:
//   bits(u), bits(i), bits(d), inside, own, bits(clamp(i)).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hrt_resolve_map.h"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

static void emit(std::vector<uint32_t>& out, uint32_t ws, uint32_t wt) {
  const uint32_t nx = hrt::resolve_phases(ws, wt);
  std::vector<float> offsets = {-0.5f, -0.25f, 0.0f, 0.25f, 0.5f};
  out.push_back(nx);
  for (uint32_t a = 0; a < nx; ++a) {
    offsets.push_back(hrt::resolve_phase_offset(a, nx));
    out.push_back(bits(offsets.back()));
  }
  for (const float off : offsets)
    for (uint32_t x = 0; x < wt; ++x) {
      const float u = hrt::resolve_coord(x, ws, wt, off);
      const float i = hrt::resolve_sample(u);
      const float d = hrt::resolve_dist(u, i);
      const uint32_t rec[6] = {bits(u), bits(i), bits(d), hrt::resolve_inside(i, ws) ? 1u : 0u,
                               hrt::resolve_own(d, ws, wt) ? 1u : 0u, bits(hrt::resolve_clamp(i, ws))};
      out.insert(out.end(), rec, rec + 6);
    }
}

int main(int argc, char** argv) {
  if (argc < 2 || argc % 2 != 0) {
    std::fprintf(stderr, "usage: %s N [ws wt]...\n", argv[0]);
    return 2;
  }
  const uint32_t n = (uint32_t)std::strtoul(argv[1], nullptr, 10);
  std::vector<uint32_t> out;
  for (uint32_t ws = 1; ws <= n; ++ws)
    for (uint32_t wt = 1; wt <= n; ++wt) emit(out, ws, wt);
  for (int a = 2; a + 1 < argc; a += 2) {
    const uint32_t ws = (uint32_t)std::strtoul(argv[a], nullptr, 10), wt = (uint32_t)std::strtoul(argv[a + 1], nullptr, 10);
    if (ws == 0 || wt == 0 || ws > (1u << 24) || wt > 16384u) return 2;
    emit(out, ws, wt);
  }
  return std::fwrite(out.data(), 4, out.size(), stdout) == out.size() ? 0 : 1;
}
