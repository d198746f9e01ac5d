// hrt_history_fold.h -- the per-pixel device functions of the temporal history's fold:
// the combiner with a pixel's own frame number, the moments step and S14's surface key of a hit record.  Shared by
// fold_history[_moments] (hrt_history.hip) and the adaptive refinement's folds and selection (hrt_refine.hip), so
// the two units fold with one spelling.  Device code only; units that include it are built with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hrt_math.h"
#include "hrt_variance.h"

namespace hrt {

// ---- the history fold ------------------------------------------------------------------------------------
// The combiner's fold for one pixel, as hrt_image.hip's accumulate<T> computes it (that unit keeps its device
// functions to itself): image_combiner.glsl's (new + cur * float(n)) / float(n + 1), in RGBA8 mode through S7
// with the three quotients taken through the denominator's reciprocal (rcp_core / div_core: the correctly
// rounded quotient on the whole range, the IEEE '/' outside it).  Both are held to tests/image_ref.py's
// fold_rgba8 / fold_rgba32f bit for bit, so they cannot drift apart unnoticed.  n >= 1 here.
__device__ __forceinline__ float4 hist_fold(float4 p, float4 n, uint32_t frame, const float*) {
  const float ff = (float)frame, ff1 = (float)(frame + 1u);
  return make_float4((n.x + p.x * ff) / ff1, (n.y + p.y * ff) / ff1, (n.z + p.z * ff) / ff1, 1.0f);
}
__device__ __forceinline__ uint32_t hist_fold(uint32_t pv, uint32_t nv, uint32_t frame, const float* tab) {
  const float ff = (float)frame, ff1 = (float)(frame + 1u);
  uint32_t out = 255u << 24;
  if (__builtin_expect(!(ff1 >= 0x1p-40f && ff1 <= 0x1p40f), 0)) {  // frame + 1 wrapped to 0
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float prev = tab[(pv >> (8 * ch)) & 255u];
      const float nc = tab[(nv >> (8 * ch)) & 255u];
      out |= unorm8((nc + prev * ff) / ff1) << (8 * ch);
    }
    return out;
  }
  const float y = rcp_core(ff1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float prev = tab[(pv >> (8 * ch)) & 255u];
    const float nc = tab[(nv >> (8 * ch)) & 255u];
    out |= unorm8(div_core(nc + prev * ff, ff1, y)) << (8 * ch);
  }
  return out;
}
// A pixel without history: the trace texel with the accumulator's alpha.
__device__ __forceinline__ float4 hist_first(float4 n) { return make_float4(n.x, n.y, n.z, 1.0f); }
__device__ __forceinline__ uint32_t hist_first(uint32_t n) { return (n & 0x00FFFFFFu) | (255u << 24); }

template <typename T>
__device__ __forceinline__ T hist_step(T cur, T nw, uint32_t n, const float* tab) {
  return n == 0u ? hist_first(nw) : hist_fold(cur, nw, n, tab);
}
__device__ __forceinline__ uint32_t hist_next(uint32_t n, uint32_t max_history) {  // min(n + 1, max) without the wrap
  return n >= max_history ? max_history : n + 1u;
}

// ---- the history fold with moments (S16) -------------------------------------------------------------------
// S14's C0 of a trace texel through the workgroup's UNORM8 table (its entries are unorm8_to_float's values).
__device__ __forceinline__ f3 texel_c0(uint32_t v, const float* tab) {
  return {tab[v & 255u], tab[(v >> 8) & 255u], tab[(v >> 16) & 255u]};
}
__device__ __forceinline__ f3 texel_c0(float4 v, const float*) { return {v.x, v.y, v.z}; }
// The moments of one pixel after the frame whose trace texel is nw: the sample (l, l * l) folded as two channels
// of a float texel are (n == 0: the sample itself, m not read by the caller).
template <typename T>
__device__ __forceinline__ float2 moments_step(float2 m, T nw, uint32_t n, const float* tab) {
  const f3 c = texel_c0(nw, tab);
  const float l = variance_lum(c.x, c.y, c.z);
  const float l2 = l * l;
  if (n == 0u) return make_float2(l, l2);
  const float ff = (float)n, ff1 = (float)(n + 1u);
  return make_float2((l + m.x * ff) / ff1, (l2 + m.y * ff) / ff1);
}

// S14's surface key of a hit record's first 16 bytes {t, kind, index, mesh}.
__device__ __forceinline__ uint32_t hist_key(float4 a) {
  const uint32_t kind = __float_as_uint(a.y), index = __float_as_uint(a.z), mesh = __float_as_uint(a.w);
  if (kind == 1u) return 0x80000000u | (index & 0x7FFFFFFFu);
  if (kind == 2u) return (mesh + 1u) & 0x7FFFFFFFu;
  return 0u;
}

}  // namespace hrt
