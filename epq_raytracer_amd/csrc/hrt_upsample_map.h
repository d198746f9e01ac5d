// hrt_upsample_map.h -- the coordinate arithmetic of the guided upsample (hrt_upsample / hrt_upsample_present;
// DESIGN.md §2 S19, §34), shared by the kernels (hrt_upsample.hip) and a plain C++ test program
// (tests/cpp/upsample_map_test.cpp): no HIP header is needed to compile it.
//
// Every function is S19's arithmetic for one axis: one rounded binary32 operation per written operation, in the
// written order.  Both users are built with -ffp-contract=off (upsample_weight is a multiply, then a subtraction).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HRT_UPMAP_FN __host__ __device__ inline
#else
#define HRT_UPMAP_FN inline
#endif

namespace hrt {

// The low-image coordinate of target pixel x's centre: ((float(x) + 0.5f) * float(ws)) / float(wt) - 0.5f.
HRT_UPMAP_FN float upsample_coord(uint32_t x, uint32_t ws, uint32_t wt) {
  const float c = (float)x + 0.5f;
  const float s = c * (float)ws;
  const float q = s / (float)wt;
  return q - 0.5f;
}

// x0 = floorf(u): the tap with offset 0.
HRT_UPMAP_FN float upsample_first(float u) { return floorf(u); }

// The tap offsets of a footprint, first and last: {0, 1} for 2, {-1, 0, 1, 2} for 4.
HRT_UPMAP_FN constexpr int upsample_tap_lo(int footprint) { return footprint == 2 ? 0 : -1; }
HRT_UPMAP_FN constexpr int upsample_tap_hi(int footprint) { return footprint == 2 ? 1 : 2; }

// inv_r: 1.0f for footprint 2, 0.5f for footprint 4.
HRT_UPMAP_FN constexpr float upsample_inv_r(int footprint) { return footprint == 2 ? 1.0f : 0.5f; }

// Whether tap coordinate xj (x0 + offset, still a float) lies inside a ws-wide image: tested in float, before
// any conversion (S15's rule), so that a coordinate no integer type holds is never converted.
HRT_UPMAP_FN bool upsample_inside(float xj, uint32_t ws) { return xj >= 0.0f && xj <= (float)(ws - 1u); }

// wx = 1.0f - fabsf(u - xj) * inv_r: the tent of radius 1 / inv_r around u.
HRT_UPMAP_FN float upsample_weight(float u, float xj, float inv_r) {
  const float d = fabsf(u - xj);
  const float m = d * inv_r;
  return 1.0f - m;
}

// The fallback's texel: ((2x+1) ws) div (2 wt), hrt_present's nearest rule (x < wt, so the result is < ws).
HRT_UPMAP_FN uint32_t upsample_nearest(uint32_t x, uint32_t ws, uint32_t wt) {
  return (uint32_t)(((2ull * x + 1ull) * ws) / (2ull * wt));
}

}  // namespace hrt
