// hrt_present_map.h -- the index arithmetic of the gathered present pass (hrt_present on the root of an
// hrt_comm_init_all group), shared by the kernels (hrt_image.hip present_rows / present_nearest) and a plain C++
// test program (tests/cpp/present_map_test.cpp): no HIP header is needed to compile it.
//
// The sampling rule is the one pinned for hrt_present (include/hip_raytrace.h): sample
// points at the target's pixel centres, nearest filter, flipped vertically, 64-bit intermediates so
// that no size up to 16384 x 16384 overflows.  The row map is the row-tile partition's (hip_raytrace.h
// hrt_create_info): global row y lives in part (y / row_tile) % parts at local row
// (y / row_tile / parts) * row_tile + y % row_tile; the root's gather buffer holds the parts' blocks of
// local_rows rows each in part order.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HRT_MAP_FN __host__ __device__ inline
#else
#define HRT_MAP_FN inline
#endif

namespace hrt {

// Source column of target column x: ((2x+1) ws) div (2 wt)   (x < wt, so the result is < ws).
HRT_MAP_FN uint32_t present_sx(uint32_t x, uint32_t ws, uint32_t wt) {
  return (uint32_t)(((2ull * x + 1ull) * ws) / (2ull * wt));
}

// Source row of target row y: hs - 1 - ((2y+1) hs) div (2 ht)   (y < ht, so the result is in [0, hs)).
HRT_MAP_FN uint32_t present_sy(uint32_t y, uint32_t hs, uint32_t ht) {
  return hs - 1u - (uint32_t)(((2ull * y + 1ull) * hs) / (2ull * ht));
}

// Row of the rank-major gather buffer (parts blocks of local_rows rows) that holds global row y:
// part * local_rows + local row.  64-bit: the caller multiplies it by the row's bytes.
HRT_MAP_FN uint64_t gathered_row(uint32_t y, uint32_t row_tile, uint32_t parts, uint32_t local_rows) {
  const uint32_t t = y / row_tile;
  return (uint64_t)(t % parts) * local_rows + (uint64_t)(t / parts) * row_tile + y % row_tile;
}

}  // namespace hrt
