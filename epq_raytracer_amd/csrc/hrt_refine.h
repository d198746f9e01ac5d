// hrt_refine.h -- launch interface of the adaptive refinement (hrt_refine.hip): the
// selection of the pixels whose estimate is still noisy (hrt_refine_select), and the pieces of one refinement
// pass over a selection mask (hrt_refine): the compact list of radiance queries, the fold of their results into
// the selected pixels, and the masked fold of a whole traced frame.
//
// The mask is hrt_occluded's layout over i = x + y W: pixel i is bit i & 31 of word i >> 5, ceil(npix / 32) words.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_raytrace.h"

namespace hrt {

// What the selection kernel takes of an hrt_refine_rule: tol2 = tolerance * tolerance, one rounded product.
struct RefineRuleK {
  uint32_t min_history, max_count, radius;
  float tol2, luminance_floor;
};

// mask <- S17's selection over a w x h image from the count image, the moments image and, when hits is not null,
// the surface keys of w x h hrt_hit records (16-byte aligned); every word written in full, the unused high bits of
// the last word 0.  *selected (zeroed by the caller) += the number of selected pixels.
hipError_t launch_refine_select(const uint32_t* cnt, const float* mom, const hrt_hit* hits, uint32_t* mask,
                                unsigned long long* selected, uint32_t w, uint32_t h, const RefineRuleK& rule,
                                hipStream_t stream);

// The selected pixels of mask as a compact list: entry e holds the pixel index[e] = i and its radiance query
// queries[2 e], queries[2 e + 1] = (cam_pos, seed_base + i), (ray centre i, 0).  *next (zeroed by the caller)
// += the entries.  queries == null: the count alone.  The order of the entries is free.  Lists: npix entries.
hipError_t launch_refine_queries(const uint32_t* mask, const float4* rays, float4* queries, uint32_t* index,
                                 uint32_t* next, uint32_t npix, const float cam_pos[3], uint32_t seed_base,
                                 hipStream_t stream);

// For every entry e < n: the texel of rgba[e] (in RGBA8 mode through S7's store, alpha 255) folded into pixel
// index[e] of cur / cnt (/ mom when not null) as launch_fold_history[_moments] folds a trace texel.
hipError_t launch_refine_fold(void* cur, uint32_t* cnt, float* mom, bool f32, const float4* rgba, const uint32_t* index,
                              uint32_t n, uint32_t max_history, hipStream_t stream);

// launch_fold_history[_moments] for the pixels whose bit is set in mask; every other pixel is left alone.
hipError_t launch_refine_fold_image(void* cur, const void* nw, uint32_t* cnt, float* mom, bool f32, const uint32_t* mask,
                                    uint32_t npix, uint32_t max_history, hipStream_t stream);

// ---- the tile-masked pass (hrt_refine_tiles) ----
// bits <- one bit per 8x8 tile of a w x h image, set when any real pixel of the tile has its mask bit set:
// ceil(tiles / 32) words, each written in full, the unused high bits of the last word 0.  counts[0..2] (zeroed by
// the caller) += the set bits of real pixels, the selected tiles, the real pixels of the selected tiles.
hipError_t launch_refine_tile_bits(const uint32_t* mask, uint32_t* bits, unsigned long long* counts, uint32_t w, uint32_t h,
                                   hipStream_t stream);

// The planner's histogram and fill passes over the selected tiles (hrt_kernels.hip's plan_hist / plan_fill otherwise;
// plan_scan runs between them).  cost: a previous trace's tile costs, or null: 1 for every tile.  sched's histogram,
// cursors and words 6..7 are zeroed by the caller; the histogram pass adds the selected tiles' costs to words 6..7.
hipError_t launch_plan_hist_masked(uint32_t* sched, const uint32_t* cost, const uint32_t* bits, uint32_t tiles,
                                   const uint32_t* tl_cache, hipStream_t stream);
hipError_t launch_plan_fill_masked(uint32_t* sched, const uint32_t* cost, const uint32_t* bits, uint32_t tiles, uint32_t kmax,
                                   uint32_t prio, uint32_t* items, const uint32_t* tl_cache, hipStream_t stream);

// launch_refine_fold_image for the nf frames at stack + f * stride pixels, f = 0 .. nf - 1 in order, in one pass.
// trace (may be null; then tile_bits is not read): every pixel whose tile's bit is set gets frame nf - 1's texel.
hipError_t launch_refine_fold_frames(void* cur, const void* stack, size_t stride, uint32_t nf, uint32_t* cnt, float* mom,
                                     bool f32, const uint32_t* mask, const uint32_t* tile_bits, void* trace, uint32_t w,
                                     uint32_t h, uint32_t max_history, hipStream_t stream);

}  // namespace hrt
