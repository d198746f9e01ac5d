// hrt_history.h -- launch interface of the temporal history (hrt_history.hip): the
// combiner with a per-pixel frame number (hrt_accumulate_history) and the pass that carries accumulator and
// count image from one view to the next through the two views' first hits (hrt_reproject).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_raytrace.h"

namespace hrt {

constexpr uint32_t kHistoryMax = HRT_HISTORY_MAX;  // the largest max_history: float(n) is exact up to here

// cur[i] <- the fold of trace texel nw[i] into accumulator texel cur[i] with the pixel's own frame number
// n = cnt[i] (n == 0: the trace texel with alpha 255 / 1.0f, cur[i] not read); cnt[i] <- min(n + 1, max_history).
// f32: float4 texels (16-byte aligned), else packed RGBA8 words.
hipError_t launch_fold_history(void* cur, const void* nw, uint32_t* cnt, bool f32, size_t npix, uint32_t max_history,
                               hipStream_t stream);

// One reprojection over a w x h image: (acc_out, cnt_out) <- S15 of (acc_in, cnt_in).  The outputs must not
// overlap the inputs.  Hit arrays: w x h hrt_hit records, 16-byte aligned.
struct ReprojectPass {
  const void* acc_in;
  const uint32_t* cnt_in;
  void* acc_out;
  uint32_t* cnt_out;
  const hrt_hit* prev_hits;
  const hrt_hit* cur_hits;
  hrt_view prev, cur;
  bool f32;
  uint32_t filter;  // hrt_reproject_filter
  uint32_t w, h;
  float depth_tolerance, min_normal_dot;
};
hipError_t launch_reproject(const ReprojectPass& p, hipStream_t stream);

// The reprojection under object motion (hrt_reproject_motion[_moments]): S15 with the
// pixel's object taken through its entry of the tables.  The tables are hrt_motion records in device memory,
// 16-byte aligned, that stay unchanged until the pass has run; a count of 0 needs no pointer.  mom_in / mom_out:
// both null (hrt_reproject_motion) or the moments images as launch_reproject_moments takes them.
struct MotionTables {
  const hrt_motion* spheres;
  const hrt_motion* meshes;
  uint32_t n_spheres, n_meshes;
};
hipError_t launch_reproject_motion(const ReprojectPass& p, const MotionTables& motion, const float* mom_in, float* mom_out,
                                   hipStream_t stream);

}  // namespace hrt
