// hrt_launch_plan.h -- which kernel a trace or query launch runs, with what workgroups, dynamic LDS and
// pair stacks, and how its heavy tiles split: everything about a launch that is arithmetic on the scene's
// sizes.  HIP-free and header-only, shared by the launch wrappers (hrt_kernels.hip), the C-ABI
// layer (hrt_api.cpp) and a plain C++ test program (tests/cpp/launch_plan_test.cpp, tests/test_launch_plan.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "hip_raytrace.h"

namespace hrt {

// What selection reads of a launch's TraceParams (hrt_kernels.hip plan_scene fills it).
struct PlanScene {
  uint32_t n_tris, cam_list_capacity;
  int32_t num_meshes, max_bounces;
  bool bvh_nodes, bvh_entries, bvh_wq_nodes, bvh_wq_nodes_bfs;  // the device images that exist
  uint32_t bvh_sah_milli, bvh_n_nodes, bvh_n_prims, bvh_n_meshes;
  uint32_t bvh_wq_n_nodes, bvh_wq_width, bvh_max_leaf, bvh_node_r;
  int32_t wq_lds_nodes_opt;   // HRT_OPT_WQ_LDS_NODES (-1: auto)
  uint32_t wq_ncap, wq_tcap;  // HRT_OPT_WQ_NODE_CAP / HRT_DEBUG_OPT_WQ_TRI_CAP requests (0: none)
};

constexpr size_t kMaxLdsScene = 160 * 1024 - 64;  // dynamic LDS per CU, leaving room for the kernels' static LDS
constexpr uint32_t kAutoCullTris = 256;   // BUNDLE_CULL from this many mesh triangles, BUNDLE below
constexpr uint32_t kAutoBvhTris = 4096;   // BUNDLE_BVH from this many (profiles/r01d_bvh_scaling.log)
constexpr uint32_t kAutoWqStack = 384;    // BUNDLE_WQ when its per-wave node stacks hold this many entries
constexpr uint32_t kAutoLeafWqStack = 512;  // auto leaf size: the smallest leaf whose image leaves this much
constexpr uint32_t kWqSlots = 4;  // widest node group the pair kernels test per stack entry (hrt_kernels.hip)

// BUNDLE_BVH_LDS footprint: triangles + nodes + entries + key bases.
inline size_t bvh_lds_bytes(const PlanScene& s) {
  return (size_t)s.n_tris * 48 + (size_t)s.bvh_n_nodes * 64 + (size_t)s.bvh_n_prims * 4 + (size_t)s.bvh_n_meshes * 4;
}

// BUNDLE_CULL_LDS workgroup size for a scene of n triangles (0 = does not fit): two 512-thread
// workgroups per CU when twice the footprint fits the 160 KiB, else one of 1024.
constexpr size_t kCoopLds = 3 * 64 * 8;  // cooperative-tile exchange slots
inline uint32_t lds_block(uint32_t n) {
  const size_t tri = (size_t)n * 48 + kCoopLds;
  return tri <= kMaxLdsScene / 2 ? 512u : tri <= kMaxLdsScene ? 1024u : 0u;
}

// BUNDLE_WQ per-wave pair stacks.  Triangle stack: 64 x (1 + 2 x largest leaf) pairs -- a node step's pushes
// onto < 64 waiting ones when each lane keeps at most two leaves; a larger burst of a grouped step is tested in place.
constexpr uint32_t wq_tri_cap(uint32_t max_leaf) { return 64u * (1u + 2u * max_leaf); }
// Node stack: what is left of the 160 KiB after the image's n_nodes records (groups of `width`, leaves of at
// most max_leaf triangles), at most 1024 pairs, at least 128; 0: does not fit the LDS
inline uint32_t wq_stack_cap(uint32_t n_nodes, uint32_t width, uint32_t max_leaf) {
  if (max_leaf > 4 || width > kWqSlots || width < 2) return 0;
  const size_t nodes = (size_t)n_nodes * 48, t = wq_tri_cap(max_leaf);
  if (nodes + 16 * (512 + 4 * (t + 128)) > kMaxLdsScene) return 0;
  const size_t per_wave = (kMaxLdsScene - nodes) / 16;
  return (uint32_t)std::min<size_t>(1024, ((per_wave - 512 - 4 * t) / 4) & ~(size_t)63);
}
// A stack capacity under its request (HRT_OPT_WQ_NODE_CAP, HRT_DEBUG_OPT_WQ_TRI_CAP; 0: none): whole
// 64-entry steps, never below 128.
inline uint32_t wq_capped(uint32_t cap, uint32_t request) {
  return request ? std::min(cap, std::max(128u, request & ~63u)) : cap;
}
// The pair stacks beside the whole node image (BUNDLE_WQ, the PAIRS query): the LDS bytes, 0 = no fit, and the
// capacities they are sized for -- the requests lower what the kernel is told (wq_capped), not the bytes.
inline size_t wq_lds_bytes(const PlanScene& s, uint32_t& ncap, uint32_t& tcap) {
  ncap = s.bvh_nodes && s.bvh_wq_nodes ? wq_stack_cap(s.bvh_wq_n_nodes, s.bvh_wq_width, s.bvh_max_leaf) : 0u;
  tcap = wq_tri_cap(s.bvh_max_leaf);
  return ncap ? (size_t)s.bvh_wq_n_nodes * 48 + 16 * (512 + 4 * ((size_t)ncap + tcap)) : 0;
}

// BUNDLE_WQ_L2's LDS plan for a breadth-first image of n_nodes records: out = {L, ncap, tcap, bytes} -- the
// slots kept in LDS, the per-wave node / triangle pair stack capacities and the dynamic LDS bytes
// L x 48 + 16 x (512 + 4 x (ncap + tcap)); bytes = 0 (all four 0): no fit (the stacks alone do not fit, or
// the image's shape is not the kernel's).  lds_nodes (HRT_OPT_WQ_LDS_NODES) < 0, auto: the stacks get
// their BUNDLE_WQ maximum first (1024 node pairs, wq_tri_cap triangle pairs; lower when ncap_req / tcap_req,
// the HRT_OPT_WQ_NODE_CAP / HRT_DEBUG_OPT_WQ_TRI_CAP requests, ask for less) and the nodes what is left.
// lds_nodes >= 0: L = min(lds_nodes, n_nodes, what fits beside stacks of the minimum 128 node pairs), and
// the node stacks what is left of the 160 KiB, up to the same maximum.
inline void wq_l2_plan(uint32_t n_nodes, uint32_t width, uint32_t max_leaf, int64_t lds_nodes, uint32_t ncap_req,
                       uint32_t tcap_req, uint32_t out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  if (n_nodes == 0 || n_nodes >= 0x10000u || max_leaf == 0 || max_leaf > 4 || width > kWqSlots || width < 2) return;
  const size_t t = wq_capped(wq_tri_cap(max_leaf), tcap_req), nmax = wq_capped(1024u, ncap_req);
  auto stacks = [&](size_t ncap) { return 16 * (512 + 4 * (ncap + t)); };
  if (stacks(128) > kMaxLdsScene) return;
  size_t L, ncap;
  if (lds_nodes < 0) {
    ncap = nmax;
    while (stacks(ncap) > kMaxLdsScene) ncap -= 64;  // (ends at 128 at the latest)
    L = std::min<size_t>(n_nodes, (kMaxLdsScene - stacks(ncap)) / 48);
  } else {
    L = std::min<size_t>({(size_t)lds_nodes, (size_t)n_nodes, (kMaxLdsScene - stacks(128)) / 48});
    const size_t per_wave = (kMaxLdsScene - L * 48) / 16;
    ncap = std::min(nmax, ((per_wave - 512 - 4 * t) / 4) & ~(size_t)63);
  }
  out[0] = (uint32_t)L;
  out[1] = (uint32_t)ncap;
  out[2] = (uint32_t)t;
  out[3] = (uint32_t)(L * 48 + stacks(ncap));
}

// One row per hrt_kernel value: what the host has to know about a trace kernel family.
struct KernelTraits {
  bool persistent;      // one or two workgroups per CU take tiles from the planner's queue and record their costs
  bool camera_lists;    // its launch (re)builds the lane's camera lists (LITERAL, BRUTE, BRUTE_LDS neither build nor read them)
  bool hierarchy;       // traverses the hierarchy: needs one, and at most 64 meshes (a ray's mesh filter is 64 bits)
  bool sky_lane;        // can run a planned launch's sky items on trace_sky beside it (HRT_OPT_SKY_LANE)
  bool pair_traversal;  // pair stacks in LDS; heavy tiles split by pair_split
  int fallback;         // what runs when the scene does not fit it (kernel_fits); itself: every scene fits
  uint32_t split_k;     // items per heavy tile when HRT_OPT_SPLIT is auto (1: none; BUNDLE_CULL_LDS runs them cooperatively)
  // bounce batch threshold, auto: the pair traversal's step cost scales with its rays, so BUNDLE_WQ
  // batches earlier (28 of 64 lanes); the cull kernels test every survivor for the whole wave (48)
  // (profiles/r01q_sec_batch_sweep.jsonl, frames in 16-frame launches); 36 for the per-node-radius
  // kernel, whose scenes bounce far more (cave 20 / 28 / 36 / 44 / 56: 7.43 / 7.38 / 7.31 / 7.32 /
  // 7.45 ms; island stays best at 28: profiles/r02v_ab.txt)
  uint32_t sec_batch, sec_batch_node_r;
  // primary threshold, auto (HRT_OPT_PRIMARY_BATCH): ready lanes from which a trip that runs a bounce batch
  // runs the primary phase too.  1 is the schedule without it.  BUNDLE_WQ: 48 at its bounce thresholds
  // (profiles/phase_batch_bench_ab.txt): against the parent, interleaved, island 2.4% and cave 1.2%
  // faster at the bench's medians and faster in every pair of runs, where 1 -- the parent's schedule in the
  // restructured loop -- measured 1.4% slower on island.  Above 64 - 28 the phases alternate strictly, so 40
  // counts the same.  The pair 40 / 36 (40 / 44 with per-node radii) gains 4.7% in 20-frame launches and needs the
  // bounce thresholds above changed with it: a change of its own.  The other rows were not measured and keep 1
  uint32_t prim_batch, prim_batch_node_r;
};
constexpr int kNumKernels = HRT_KERNEL_BUNDLE_WQ_L2 + 1;
inline constexpr KernelTraits kKernelTraits[kNumKernels] = {
    // persist lists  hier   sky    pairs  fallback                  split_k sec_batch prim_batch
    {false, false, false, false, false, HRT_KERNEL_AUTO, 1, 48, 48, 1, 1},  // AUTO (plan_trace's ladder picks a row)
    {false, false, false, false, false, HRT_KERNEL_LITERAL, 1, 48, 48, 1, 1},
    {false, false, false, false, false, HRT_KERNEL_BRUTE, 1, 48, 48, 1, 1},
    {false, false, false, false, false, HRT_KERNEL_BRUTE, 1, 48, 48, 1, 1},             // BRUTE_LDS
    {false, true, false, false, false, HRT_KERNEL_BUNDLE, 1, 48, 48, 1, 1},
    {false, true, false, false, false, HRT_KERNEL_BUNDLE_CULL, 1, 48, 48, 1, 1},
    {false, true, true, false, false, HRT_KERNEL_BUNDLE_CULL, 1, 48, 48, 1, 1},          // BUNDLE_BVH
    {true, true, false, false, false, HRT_KERNEL_BUNDLE_CULL, 1, 48, 48, 1, 1},          // BUNDLE_CULL_LDS
    {true, true, true, false, false, HRT_KERNEL_BUNDLE_BVH, 1, 48, 48, 1, 1},            // BUNDLE_BVH_LDS
    {true, true, true, true, true, HRT_KERNEL_BUNDLE_BVH_LDS, 8, 28, 36, 48, 48},        // BUNDLE_WQ
    {true, true, true, false, true, HRT_KERNEL_BUNDLE_BVH_LDS, 8, 28, 36, 1, 1},         // BUNDLE_WQ_L2
};
inline const KernelTraits& kernel_traits(int k) {
  return kKernelTraits[k >= 0 && k < kNumKernels ? k : HRT_KERNEL_BRUTE];  // (launch_trace's default is trace_brute)
}

// A trace launch, as far as the scene decides it.
struct LaunchPlan {
  int kernel;              // the hrt_kernel that runs
  uint32_t block;          // threads per workgroup: 256, 512 or 1024
  uint32_t groups_per_cu;  // persistent kernels: workgroups per CU; 0: one per 16 x 16 pixels (32 x 32 at block 1024)
  size_t lds_bytes;        // dynamic LDS
  uint32_t wq_ncap, wq_tcap, wq_lds_nodes;  // pair traversal: the stack capacities and LDS node slots the kernel is told
  uint32_t split_k, sec_batch;              // the row's defaults (sec_batch by the scene's bvh_node_r)
  uint32_t prim_batch;                      // ... and its primary threshold, chosen the same way
};

// Kernel k's launch on this scene; false: the scene does not fit it -- the only place that says so.  (The
// pair kernels' fit does not ask for the stacks AUTO wants, and BUNDLE_WQ's ignores the capacity requests.)
inline bool size_kernel(const PlanScene& s, int k, LaunchPlan& plan) {
  const KernelTraits& t = kernel_traits(k);
  plan = LaunchPlan{k, t.persistent || k == HRT_KERNEL_BRUTE_LDS ? 1024u : 256u, t.persistent ? 1u : 0u, 0, 0u, 0u, 0u,
                    t.split_k, s.bvh_node_r ? t.sec_batch_node_r : t.sec_batch,
                    s.bvh_node_r ? t.prim_batch_node_r : t.prim_batch};
  if (t.hierarchy && (!s.bvh_nodes || s.num_meshes > 64)) return false;
  uint32_t l2[4] = {0, 0, 0, 0};
  switch (k) {
    case HRT_KERNEL_BRUTE_LDS:
      plan.lds_bytes = (size_t)s.n_tris * 48;
      break;
    case HRT_KERNEL_BUNDLE_CULL_LDS:
      plan.block = lds_block(s.n_tris);
      plan.groups_per_cu = plan.block == 512 ? 2 : 1;
      plan.lds_bytes = (size_t)s.n_tris * 48 + kCoopLds;
      break;
    case HRT_KERNEL_BUNDLE_BVH_LDS:
      plan.lds_bytes = bvh_lds_bytes(s);
      return s.bvh_entries && plan.lds_bytes <= kMaxLdsScene;
    case HRT_KERNEL_BUNDLE_WQ:
      plan.lds_bytes = wq_lds_bytes(s, plan.wq_ncap, plan.wq_tcap);
      plan.wq_ncap = wq_capped(plan.wq_ncap, s.wq_ncap);
      plan.wq_tcap = wq_capped(plan.wq_tcap, s.wq_tcap);
      return plan.lds_bytes != 0;
    case HRT_KERNEL_BUNDLE_WQ_L2:
      if (s.bvh_wq_nodes_bfs)  // (the image exists and is uploaded: the context selected the variant)
        wq_l2_plan(s.bvh_wq_n_nodes, s.bvh_wq_width, s.bvh_max_leaf, s.wq_lds_nodes_opt, s.wq_ncap, s.wq_tcap, l2);
      plan.wq_lds_nodes = l2[0], plan.wq_ncap = l2[1], plan.wq_tcap = l2[2], plan.lds_bytes = l2[3];
      return plan.lds_bytes != 0;
  }
  return plan.lds_bytes <= kMaxLdsScene;
}
// A launch's batch threshold (HRT_OPT_SECONDARY_BATCH, HRT_OPT_PRIMARY_BATCH): the request, or the plan's when it is 0
inline uint32_t batch_threshold(uint32_t request, uint32_t planned) { return request ? request : planned; }
inline bool kernel_fits(const PlanScene& s, int k) { LaunchPlan plan; return size_kernel(s, k, plan); }

inline LaunchPlan plan_trace(const PlanScene& s, int k) {  // k: the hrt_kernel requested
  if (k == HRT_KERNEL_AUTO) {
    // profiles/r01g_*: island 21.4 (LDS) vs 23.7 ms, cave 112 vs 120 ms; BVH from ~4K triangles.
    // BUNDLE_WQ when its node stacks get >= kAutoWqStack entries (r02, node groups: island 2.84 vs
    // ~15 ms for BUNDLE_CULL_LDS; cave 17.3 ms at 384-entry stacks vs 20.2, profiles/r02p_cave_wq.txt)
    // A poor hierarchy (large overlapping triangles, HRT_SCENE_BVH_SAH_MILLI > 100) is left to the
    // wave-level culls: triangle soups of 256 / 1K / 4K / 16K run 2.5-5x faster culled
    // (profiles/r01p_soup_sweep.log).
    const bool good_bvh = s.bvh_nodes && s.bvh_sah_milli <= 100;
    const bool wq = good_bvh && kernel_fits(s, HRT_KERNEL_BUNDLE_WQ) &&
                    wq_stack_cap(s.bvh_wq_n_nodes, s.bvh_wq_width, s.bvh_max_leaf) >= kAutoWqStack;
    k = s.cam_list_capacity < kAutoCullTris               ? HRT_KERNEL_BUNDLE
        : wq                                              ? HRT_KERNEL_BUNDLE_WQ
        : s.cam_list_capacity >= kAutoBvhTris && good_bvh ? HRT_KERNEL_BUNDLE_BVH
        : kernel_fits(s, HRT_KERNEL_BUNDLE_CULL_LDS)      ? HRT_KERNEL_BUNDLE_CULL_LDS
                                                          : HRT_KERNEL_BUNDLE_CULL;
  }
  LaunchPlan plan;
  // (every chain ends in a row that is its own fallback and fits every scene)
  while (!size_kernel(s, k, plan)) k = kernel_traits(k).fallback;
  if (s.max_bounces < 0) size_kernel(s, HRT_KERNEL_LITERAL, plan);  // the fused loops assume >= 1 segment per path
  return plan;
}

// A ray-query launch: the method an hrt_query_method request runs on the scene (AUTO resolved, fallbacks
// applied: the traversals are the trace kernels', with their fit rules) and, for PAIRS, BUNDLE_WQ's stacks.
struct QueryPlan {
  int method;
  size_t lds_bytes;
  uint32_t wq_ncap, wq_tcap;
};
inline QueryPlan plan_query(const PlanScene& s, int method) {
  LaunchPlan wq{};
  if (method == HRT_QUERY_AUTO) method = HRT_QUERY_BVH;
  if (method == HRT_QUERY_PAIRS && !size_kernel(s, HRT_KERNEL_BUNDLE_WQ, wq)) method = HRT_QUERY_BVH;
  if (method == HRT_QUERY_BVH && !kernel_fits(s, HRT_KERNEL_BUNDLE_BVH)) method = HRT_QUERY_SCAN;
  return method == HRT_QUERY_PAIRS ? QueryPlan{method, wq.lds_bytes, wq.wq_ncap, wq.wq_tcap} : QueryPlan{method, 0, 0u, 0u};
}

// Heavy tiles: those that cost more than factor x a resident wave's fair share of the launch run as split_k items.
// The pair traversal's rule for an auto (< 0) HRT_OPT_SPLIT_FACTOR request:
// a pair step's work scales with the rays in the batch, so heavy tiles (> factor x a
// resident wave's fair share of the work) run as 2, 4 or 8 items by cost; factor 2 when a
// resident wave gets more than 6 tiles (the full frame), else 3 (row partitions at N > 1)
// (profiles/r01o_lane_weighted_sum_factor_sweep.jsonl)
// A launch of several frames (hrt_compute_n) splits a tile from 1.25 x a wave's share of the launch:
// a rank of 8 holds 1/8 of the rows but the same pixel chains, and one cave tile's frame took 18 ms
// against a 15 ms share, unsplit at 2 x (profiles/r06/r06aa/).  Cave's slowest rank of 8 0.88 ->
// 0.80 ms per frame; island, 2 and 4 ranks and whole frames within noise (r06ac, r06ad).
struct SplitFactor {
  int32_t factor;    // TraceParams::split_factor
  uint32_t factor4;  // TraceParams::split_factor4: quarters of a share; 0: factor
};
inline SplitFactor pair_split(uint32_t tiles, uint32_t n_frames, uint32_t num_cus, int32_t request) {
  if (request >= 0) return {request, 0u};
  if (n_frames > 1) return {request, 5u};
  return {(uint64_t)tiles * std::max(1u, n_frames) > 6ull * num_cus * 16u ? 2 : 3, 0u};
}
// The planner's (prepare_schedule): a resident wave's fair share of a launch of nf frames is nf frames' work, i.e.
// waves / nf per frame
inline uint32_t plan_waves(uint32_t num_cus, uint32_t nf) { return std::max(1u, num_cus * 16u / std::max(1u, nf)); }
// factor auto (-1): 3 when a resident wave gets more than 4 tiles, else 1 (profiles/r01k_schedule_sweep)
inline uint32_t plan_factor4(uint32_t tiles, uint32_t waves, const SplitFactor& f) {
  return f.factor4 ? f.factor4 : 4u * (f.factor >= 0 ? (uint32_t)f.factor : tiles > 4 * waves ? 3u : 1u);
}

}  // namespace hrt
