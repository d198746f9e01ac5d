// hrt_resolve.h -- launch interface of the fold across resolutions (hrt_resolve.hip): the
// pass hrt_accumulate_history_from runs to fold a ws x hs trace image, sampled on a grid shifted by a fraction of a
// pixel, into the w x h accumulator, count image and moments image of a context of another size.
//
// One call is one kernel, resolve<T, Moments, Guided>: a lane per target pixel finds the one source sample that
// can lie in its pixel, takes one hrt_accumulate_history[_moments] step with it when it does (and, guided, when
// both first hits carry one surface key), and otherwise leaves the pixel alone -- or, asked to fill, shows the
// nearest source texel in a pixel that has no history yet.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_raytrace.h"

namespace hrt {

struct ResolvePass {
  void* acc;                 // w x h texels of the context's format (float4: 16-byte aligned): A
  uint32_t* cnt;             // w x h counts: N
  float* mom;                // w x h float pairs, 8-byte aligned: M (nullptr: the moments are not folded)
  const void* src;           // ws x hs texels of the same format: T
  const hrt_hit* src_hits;   // ws x hs records, 16-byte aligned, or nullptr with hits (unguided)
  const hrt_hit* hits;       // w x h records, 16-byte aligned
  bool f32;
  uint32_t ws, hs, w, h;     // each 1..2^24: float(ws - 1) is exact
  float offset_x, offset_y;  // finite
  uint32_t max_history;      // 1..2^24
  uint32_t fill;             // HRT_RESOLVE_FILL
};
// src and the hit arrays must not overlap acc, cnt and mom.
hipError_t launch_resolve(const ResolvePass& p, hipStream_t stream);

}  // namespace hrt
