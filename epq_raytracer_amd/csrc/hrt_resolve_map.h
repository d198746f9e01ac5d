// hrt_resolve_map.h -- the coordinate arithmetic of the fold across resolutions (hrt_accumulate_history_from;
// DESIGN.md §2 S20, §35) and of hrt_history_phase, shared by the kernels (hrt_resolve.hip), the host entry point
// (hrt_api.cpp) and a plain C++ test program (tests/cpp/resolve_map_test.cpp): no HIP header is needed to compile it.
//
// Every function is S20's arithmetic for one axis: one rounded binary32 operation per written operation, in the
// written order.  Every user is built with -ffp-contract=off (resolve_own is two multiplies, then a comparison).
#pragma once

#include <cmath>
#include <cstdint>

#include "hrt_upsample_map.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HRT_RSMAP_FN __host__ __device__ inline
#else
#define HRT_RSMAP_FN inline
#endif

namespace hrt {

// The sample coordinate of target pixel x's centre: S19's upsample_coord(x, ws, wt) - offset (source sample i sits at
// source coordinate i + offset, so sample i is at u == i).
HRT_RSMAP_FN float resolve_coord(uint32_t x, uint32_t ws, uint32_t wt, float offset) {
  return upsample_coord(x, ws, wt) - offset;
}

// i = floorf(u + 0.5f): the sample nearest u, still a float.
HRT_RSMAP_FN float resolve_sample(float u) { return floorf(u + 0.5f); }

// Whether sample i lies inside a ws-wide image: tested in float, before any conversion (S15's rule).
HRT_RSMAP_FN bool resolve_inside(float i, uint32_t ws) { return i >= 0.0f && i <= (float)(ws - 1u); }

// d = fabsf(u - i): the distance of the sample from the pixel's centre, in source texels.
HRT_RSMAP_FN float resolve_dist(float u, float i) { return fabsf(u - i); }

// Whether the sample lies in the target pixel itself: d * float(wt) <= 0.5f * float(ws).
HRT_RSMAP_FN bool resolve_own(float d, uint32_t ws, uint32_t wt) {
  const float a = d * (float)wt;
  const float b = 0.5f * (float)ws;
  return a <= b;
}

// i clamped in float to [0, ws - 1]: the fill's texel (i is finite: the offset and the sizes are).
HRT_RSMAP_FN float resolve_clamp(float i, uint32_t ws) {
  const float hi = (float)(ws - 1u);
  return i < 0.0f ? 0.0f : (i > hi ? hi : i);
}

// hrt_history_phase for one axis: the number of phases nx = max(1, ceil(wt / ws)) and phase a's offset
// (float(a) + 0.5f) / float(nx) - 0.5f.
HRT_RSMAP_FN uint32_t resolve_phases(uint32_t ws, uint32_t wt) {
  if (ws == 0u) return 1u;
  const uint32_t n = wt / ws + (wt % ws != 0u ? 1u : 0u);
  return n > 1u ? n : 1u;
}
HRT_RSMAP_FN float resolve_phase_offset(uint32_t a, uint32_t nx) {
  const float c = (float)a + 0.5f;
  const float q = c / (float)nx;
  return q - 0.5f;
}

}  // namespace hrt
