// hrt_variance.h -- launch interface of the variance-guided denoise: the luminance
// moments image M that travels beside the temporal history's accumulator and counts (fold_history_moments and
// the moments form of reproject, both in hrt_history.hip), and the filter hrt_denoise_variance /
// hrt_denoise_variance_present run over the accumulator (hrt_variance.hip).
//
// One filter call is variance_prep (accumulator -> float4 {r, g, b, V0}, hit records -> compact guide) followed
// by one a-trous pass per iteration, ping-ponging between two float4 images whose .w carries the variance; the
// last pass writes the output form.  Both forms of a pass compute S16 with the same device functions, tap by tap
// in the same order: they differ only in where a tap's operands are read from, so they give the same bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_raytrace.h"
#include "hrt_history.h"

namespace hrt {

constexpr uint32_t kVarianceMaxIterations = 5;  // steps 1, 2, 4, 8, 16

#ifdef __HIPCC__
// S16's luminance of S14's C0, for the moments fold (hrt_history.hip) and the spatial estimate (hrt_variance.hip):
// two products, then two sums in the written order (both units are built with -ffp-contract=off).
__device__ __forceinline__ float variance_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
#endif

// Where a pass reads its taps from.
enum VarianceForm {
  kVarianceDirect = 0,  // atrous_variance_direct: one thread per pixel, every tap a global load
  kVarianceTiled = 1    // atrous_variance_tiled: a 32 x 8 tile plus its 2s halo staged in LDS (steps 1, 2, 4)
};
// The form hrt_variance_method `method` runs pass i (step 1 << i) in.  HRT_VARIANCE_TILED: the dense tile while it
// fits the LDS of a launch (steps 1, 2, 4: 15.2, 22.5, 40.5 KiB), the direct kernel above.  HRT_VARIANCE_AUTO: per
// step, what measured faster at 1080p.
inline int variance_form(uint32_t method, uint32_t i) {
  if (method == HRT_VARIANCE_TILED) return i <= 2 ? kVarianceTiled : kVarianceDirect;
  if (method == HRT_VARIANCE_DIRECT) return kVarianceDirect;
  // AUTO: the tiled kernel wins steps 1 and 2 with the ranges apart (0.048 / 0.054 ms against 0.079 / 0.095 per step);
  // at step 4 its 40.5 KiB tile leaves three workgroups a CU and the ranges overlap (0.093 against 0.097): DIRECT
  return i <= 1 ? kVarianceTiled : kVarianceDirect;
}

// launch_fold_history with the moments image: cur, nw and cnt as there; mom[i] (two floats per pixel, 16-byte
// aligned) <- the fold of (l, l * l), l = the luminance of trace texel i, with the same frame number.
hipError_t launch_fold_history_moments(void* cur, const void* nw, uint32_t* cnt, float* mom, bool f32, size_t npix,
                                       uint32_t max_history, hipStream_t stream);

// launch_reproject with the moments image: mom_out <- mom_in carried as two colour channels of a float texel are
// (the same taps, weights and order); a rejected pixel gets (0, 0).  mom_in and mom_out must not overlap.
hipError_t launch_reproject_moments(const ReprojectPass& p, const float* mom_in, float* mom_out, hipStream_t stream);

// Every pixel's moments = (m1, m2).
hipError_t launch_fill_moments(float* mom, size_t npix, float m1, float m2, hipStream_t stream);

// c0[i] <- {rgb of source texel i as float (S14's C0), V0 of S16}; with hits, also guide[i] <- {n.x, n.y, n.z, t}
// and keys[i] <- the surface key of record i (without: every key is 0).  hits, c0, guide and mom 16-byte aligned.
struct VariancePrep {
  const void* src;      // the accumulator, w x h texels of the context's format
  bool f32;
  const hrt_hit* hits;  // or null
  const uint32_t* cnt;
  const float* mom;
  void* c0;
  void* guide;
  void* keys;
  uint32_t w, h, min_history;
};
hipError_t launch_variance_prep(const VariancePrep& p, hipStream_t stream);

// What a pass, or launch_variance_store, writes.
enum VarianceOut {
  kVarianceOutPass = 0,   // float4 {r, g, b, V}: the input of the next pass
  kVarianceOutFloat = 1,  // float4 texels with alpha 1.0f
  kVarianceOutRgba8 = 2   // S7's RGBA8 words, alpha 255
};
// One a-trous pass over a w x h image: out <- S16's pass with step `step` of `in` (float4 {r, g, b, V}).  guide /
// keys null: the colour-only filter.  vout (kVarianceOutFloat / Rgba8 only; may be null): one float per pixel, the
// pass's variance.  in and out must not overlap.
struct VariancePass {
  const void* in;
  const void* guide;
  const void* keys;
  void* out;
  float* vout;
  int out_kind;  // VarianceOut
  uint32_t w, h, step;
  float sv2, variance_floor, kn, sigma_depth;  // S16's and S14's host constants
};
hipError_t launch_variance_atrous(const VariancePass& p, int form, hipStream_t stream);

// iterations == 0: out <- the texels of `in` in the output form, vout (may be null) <- their .w.
hipError_t launch_variance_store(const void* in, void* out, float* vout, int out_kind, size_t npix, hipStream_t stream);

}  // namespace hrt
