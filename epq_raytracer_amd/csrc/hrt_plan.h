// hrt_plan.h -- the device planner's helpers and the scheduler words of the persistent trace kernels (DESIGN.md
// §18, §33): the item word's fields, the layout of TraceParams::sched, the cost buckets and a heavy tile's item
// count.  Shared by the planner of a whole frame (hrt_kernels.hip plan_hist / plan_scan / plan_fill, read by
// tile_loop and trace_sky) and the masked planner of a tile-masked refinement pass (hrt_refine.hip
// plan_hist_masked / plan_fill_masked), so the two plan with one spelling.  Device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hrt_kernels.h"

namespace hrt {

// Item word: tile | log2(items of the tile) << 22 | item index s << 25 | heavy << 31 (tile_loop).
constexpr uint32_t kItemTileMask = (1u << 22) - 1u;  // planned traces need fewer than 2^22 tiles
// sched[kSchedSky]: the number of sky items the plan ends in; sched[kSchedQueue ..+1]: the u64 work queue word
// (the crossing rule is written down at tile_loop).
constexpr uint32_t kSchedSky = 1000, kSchedQueue = 1002;
static_assert(kSchedQueue + 2 <= kSchedWords && kSchedQueue % 2 == 0, "sched buffer");

#ifndef HRT_PLAN_SUB
// log2 of the planner's cost buckets per octave: eighth-octave buckets put a rank's long items nearer to
// their exact longest-first order (r06p: the slowest of ranks 3 and 6 -1.7% per run on island, -1.1% on
// cave; half-octave buckets left tiles up to 1.41x apart in arbitrary order)
#define HRT_PLAN_SUB 3
#endif
constexpr uint32_t kPlanSub = HRT_PLAN_SUB, kPlanBuckets = 32u << kPlanSub;
__device__ __forceinline__ uint32_t cost_bucket(unsigned long long c) {
  if (c < (2u << kPlanSub)) return (uint32_t)c;  // (floor(log2 c) <= kPlanSub: the value itself)
  if (c > 0xFFFFFFFFull) return kPlanBuckets;
  const uint32_t v = (uint32_t)c, l = 31 - __clz(v);  // floor(log2 c) > kPlanSub
  return min((l << kPlanSub) + ((v >> (l - kPlanSub)) & ((1u << kPlanSub) - 1u)), kPlanBuckets - 1);
}
// sched words: [8, 8 + B) histogram, [8 + B, 8 + 2B) bucket offsets, [8 + 2B, 8 + 3B) cursors
constexpr uint32_t kSchedHist = 8, kSchedOff = 8 + kPlanBuckets, kSchedCur = 8 + 2 * kPlanBuckets;
static_assert(kSchedCur + kPlanBuckets <= kSchedSky, "sched buffer");
// A tile's bucket.  With a sky lane (tl_cache: the launch's tile_lists records, a scene without spheres)
// bucket 0 holds exactly the tiles whose whole-tile item is a sky item (trace_fused_split's rule: list
// ok and empty), whatever they cost, and no other tile: the descending scan puts them at the plan's far
// end, where trace_sky takes them, and sched[kSchedHist] is their number.
__device__ __forceinline__ uint32_t plan_bucket(const uint32_t* cost, const uint32_t* tl_cache, uint32_t i) {
  const uint32_t b = cost_bucket(cost[i]);
  if (!tl_cache) return b;
  const uint32_t* rec = tl_cache + (size_t)i * kTlRecWords;
  return (rec[128] == 0u && rec[129] != 0u) ? 0u : max(b, 1u);
}
// The same rule for a cost the caller holds (the masked planner: lane costs, or 1 for every tile without them).
__device__ __forceinline__ uint32_t plan_bucket_of(uint32_t c, const uint32_t* tl_cache, uint32_t i) {
  const uint32_t b = cost_bucket(c);
  if (!tl_cache) return b;
  const uint32_t* rec = tl_cache + (size_t)i * kTlRecWords;
  return (rec[128] == 0u && rec[129] != 0u) ? 0u : max(b, 1u);
}
// Items of a heavy tile in bucket b >= hb: doubling per octave above the threshold (costs [1, 2) x
// threshold: 2 items, [2, 4): 4, ... up to 64 single pixels), at most kmax; kmax = 1: never split.
__device__ __forceinline__ uint32_t bucket_items(uint32_t b, uint32_t hb, uint32_t kmax) {
  return b < hb ? 1u : min(kmax, 2u << min((b - hb) >> kPlanSub, 5u));
}

}  // namespace hrt
