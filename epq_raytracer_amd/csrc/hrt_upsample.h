// hrt_upsample.h -- launch interface of the guided upsample (hrt_upsample.hip): the pass
// hrt_upsample / hrt_upsample_present run to show a ws x hs image at wt x ht, a joint-bilateral reconstruction
// guided by the first hits of both resolutions.
//
// One call is one kernel, upsample<Footprint, Out>: a lane per target pixel reads its own hit record from the
// high guide, its 4 or 16 taps (colour, compact guide, key) from the low image's arrays -- what denoise_prep or a
// filter left in the context's scratch -- and stores the pixel in one of three forms.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_raytrace.h"

namespace hrt {

// The form a pass stores its pixels in.
enum UpsampleOut {
  kUpsampleOutFloat = 0,   // float4 texels with alpha 1.0f, row y of the result at y * wt (16-byte aligned)
  kUpsampleOutRgba8 = 1,   // S7's RGBA8 words, alpha 255, same order
  kUpsampleOutPresent = 2  // hrt_present's equal-size target: pixel (x, ht - 1 - y) of rows `pitch` bytes apart,
                           // bytes 0 and 2 swapped when bgra
};

struct UpsamplePass {
  const void* low;        // ws x hs float4 texels (rgb read)
  const void* guide;      // ws x hs float4 {n.x, n.y, n.z, t}
  const void* keys;       // ws x hs surface keys
  const hrt_hit* high;    // wt x ht records, 16-byte aligned
  void* out;
  int out_kind;           // UpsampleOut
  uint32_t ws, hs, wt, ht;
  uint32_t pitch, bgra;   // kUpsampleOutPresent only (pitch a multiple of 4, at least wt * 4)
  uint32_t footprint;     // 2 or 4
  float kn, sigma_depth;  // S19's host constant 1.0f / sigma_normal, and sigma_depth
};
// low, guide, keys and high must not overlap out.
hipError_t launch_upsample(const UpsamplePass& p, hipStream_t stream);

}  // namespace hrt
