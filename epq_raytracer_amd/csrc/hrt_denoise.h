// hrt_denoise.h -- launch interface of the denoise pass (hrt_denoise.hip): the
// guided a-trous filter hrt_denoise / hrt_denoise_present run between the accumulator and the screen.
//
// One call is denoise_prep (source image -> float4 C0, hit records -> compact guide) followed by one
// a-trous pass per iteration, ping-ponging between two float4 images; the last pass writes the output form.
// Every form of a pass computes S14 with the same device function, tap by tap in the same order: the forms
// differ only in where a tap's operands are read from, so they give the same bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_raytrace.h"

namespace hrt {

constexpr uint32_t kDenoiseMaxIterations = 5;  // steps 1, 2, 4, 8, 16

// Where a pass reads its taps from.
enum AtrousForm {
  kAtrousDirect = 0,   // atrous_direct: one thread per pixel, every tap a global load
  kAtrousDense = 1,    // atrous_tiled: a 32 x 8 tile plus its 2s halo staged in LDS (steps 1, 2, 4: 15.2, 22.5, 40.5 KiB)
  kAtrousLattice = 2   // atrous_tiled: a 32 x 8 tile of the pixels congruent mod s plus a halo of 2 lattice points
};
// The form hrt_denoise_method `method` runs pass i (step 1 << i) in.  HRT_DENOISE_TILED: the dense tile while
// its halo is at most the tile (s <= 2), the sub-lattice above.  HRT_DENOISE_AUTO: per step, what measured
// faster at 1080p.
inline int atrous_form(uint32_t method, uint32_t i) {
  if (method == HRT_DENOISE_DIRECT) return kAtrousDirect;
  if (method == HRT_DENOISE_TILED) return i <= 1 ? kAtrousDense : kAtrousLattice;
  if (method == HRT_DEBUG_DENOISE_DENSE) return i <= 2 ? kAtrousDense : kAtrousLattice;
  if (method == HRT_DEBUG_DENOISE_LATTICE) return kAtrousLattice;
  // AUTO: the tiled kernel wins steps 1, 2 and 4 (0.058 ms against 0.082 per step), the direct kernel steps 8
  // and 16, where the sub-lattice's global loads are 128 and 256 bytes apart (0.12 / 0.17 ms against 0.08)
  return i <= 2 ? atrous_form(HRT_DENOISE_TILED, i) : kAtrousDirect;
}

// c0[i] <- the rgb of source texel i as float (S14: an RGBA8 byte k is float(k) / 255.0f); with hits, also
// guide[i] <- {n.x, n.y, n.z, t} and keys[i] <- the surface key of record i.  hits, c0 and guide 16-byte aligned.
hipError_t launch_denoise_prep(const void* src, bool f32, const hrt_hit* hits, void* c0, void* guide, void* keys,
                               size_t npix, hipStream_t stream);

// One a-trous pass over a w x h image: out <- S14's pass with step `step` of `in` (float4 texels).  guide / keys
// null: the colour-only filter.  out_rgba8: out is packed RGBA8 words (S7's store, alpha 255), else float4 texels
// with alpha 1.0f (16-byte aligned).  in and out must not overlap.
struct AtrousPass {
  const void* in;
  const void* guide;
  const void* keys;
  void* out;
  bool out_rgba8;
  uint32_t w, h, step;
  float kc, kn, sigma_depth;  // kc_i, kn and sigma_depth of S14's host constants
};
hipError_t launch_atrous(const AtrousPass& p, int form, hipStream_t stream);

}  // namespace hrt
