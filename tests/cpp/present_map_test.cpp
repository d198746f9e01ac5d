// present_map_test.cpp -- prints the gathered present's index arithmetic (epq_raytracer_amd/csrc/
// hrt_present_map.h, the functions hrt_image.hip's present kernels call) compiled as plain C++, for
// tests/test_present_gather_map.py to compare with the numpy rule (tests/present_ref.py) and the
// row-tile assembly (epq_raytracer_amd/rowtiles.py).
//
// usage: present_map_test  ws hs wt ht row_tile parts local_rows  [the same seven numbers again ...]
// One JSON line per case:
//   sx[wt], sy[ht]       present_sx / present_sy of every target column / row
//   grow[hs]             gathered_row of every global row of the source
//   trow[ht]             gathered_row(sy[y]): the gather-buffer row target row y reads
//   tbyte[ht]            trow[y] * ws * 16: its byte offset in an RGBA32F gather buffer (64-bit)
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hrt_present_map.h"

namespace {

void print_list(const char* name, const std::vector<uint64_t>& v, const char* end) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf(i ? ", %" PRIu64 : "%" PRIu64, v[i]);
  std::printf("]%s", end);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 8 || (argc - 1) % 7 != 0) {
    std::fprintf(stderr, "usage: %s ws hs wt ht row_tile parts local_rows ...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a + 6 < argc; a += 7) {
    uint32_t v[7];
    for (int i = 0; i < 7; ++i) v[i] = (uint32_t)std::strtoul(argv[a + i], nullptr, 10);
    const uint32_t ws = v[0], hs = v[1], wt = v[2], ht = v[3], row_tile = v[4], parts = v[5], local_rows = v[6];
    if (!ws || !hs || !wt || !ht || !row_tile || !parts) return 2;
    std::vector<uint64_t> sx(wt), sy(ht), grow(hs), trow(ht), tbyte(ht);
    for (uint32_t x = 0; x < wt; ++x) sx[x] = hrt::present_sx(x, ws, wt);
    for (uint32_t y = 0; y < hs; ++y) grow[y] = hrt::gathered_row(y, row_tile, parts, local_rows);
    for (uint32_t y = 0; y < ht; ++y) {
      const uint32_t s = hrt::present_sy(y, hs, ht);
      sy[y] = s;
      trow[y] = hrt::gathered_row(s, row_tile, parts, local_rows);
      tbyte[y] = trow[y] * ws * 16u;
    }
    std::printf("{\"case\": [%u, %u, %u, %u, %u, %u, %u], ", ws, hs, wt, ht, row_tile, parts, local_rows);
    print_list("sx", sx, ", ");
    print_list("sy", sy, ", ");
    print_list("grow", grow, ", ");
    print_list("trow", trow, ", ");
    print_list("tbyte", tbyte, "}\n");
  }
  return 0;
}
