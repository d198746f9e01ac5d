// hrt_kernels.h -- launch interface between the C-ABI layer (hrt_api.cpp) and the gfx950 trace kernels
// (hrt_kernels.hip); the image passes' is hrt_image.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_raytrace.h"
#include "hrt_launch_plan.h"

namespace hrt {

constexpr uint32_t kSchedWords = 1024;  // TraceParams::sched (hrt_kernels.hip kSchedHist ...)

// Kernel argument block (passed by value; lives in the kernarg segment, read through SGPRs).
struct TraceParams {
  const float4* rays;            // W*H sample centres, indexed by global pixel id
  const hrt_sphere* spheres;
  const hrt_triangle* tris;
  const hrt_mesh* meshes;
  const float4* tri_nhat;        // per triangle: normalize(normal) (tri_normals at hrt_set_scene)
  uint32_t* img8;                // local_rows x W packed RGBA8 (RGBA8 mode) or nullptr
  float4* img32;                 // local_rows x W float4 (RGBA32F mode) or nullptr
  unsigned long long* counters;  // [0] segments, [1] triangle tests, [2] wave steps; nullptr = off
  unsigned long long* diag;      // HRT_OPT_COUNTERS = 2: cull diagnostics (HRT_DIAG_*), else nullptr
  unsigned long long* tile_cycles;  // HRT_OPT_COUNTERS = 2: per 8x8 tile {clocks, bounce iterations,
                                    // bounce survivors, bounce clocks}, else nullptr
  hrt_push_constants pc;
  uint32_t local_rows, row_tile, part_index, part_count;
  uint32_t n_tris;               // uploaded triangle count (LDS staging)
  // Bundle variants: per-frame compacted camera-facing triangles (camera_lists kernel).
  uint32_t* cam_start;           // num_meshes: first compacted record of mesh m
  uint32_t* cam_count;           // num_meshes: its number of camera-facing triangles
  uint32_t cam_list_capacity;    // sum of the meshes' len (record capacity)
  float4* cam_tris;              // 4 float4 per record: (ao, num_t) (e1, index bits) (e2, -) (n, -)
  float4* cam_cull;              // 5 float4 per record: bundle-cull linear forms + margins
  uint32_t sec_batch;            // bounce segments run once this many lanes of a wave wait (1..64)
  uint32_t prim_batch;           // a trip that runs a bounce batch runs primary segments too once this many
                                 // lanes are ready for one (1..64; 1: whenever a lane is ready)
  // Persistent (LDS) variants' scheduler: sched[1] item count, [2] heavy tiles,
  // [3] first heavy cost bucket, [5] cooperative-item counter, [6..7] u64 sum of tile costs,
  // [8..) planner histogram / offsets / cursors, [1000] the plan's trailing sky items, [1002..1003] the u64
  // work queue word (kSchedWords in all); tile_cost per 8x8 tile (shader clocks / 16, this trace);
  // item_buf (tiles x 8) the planned items; items = item_buf when this trace follows a plan.
  uint32_t* sched;
  uint32_t* tile_cost;
  uint32_t* item_buf;
  const uint32_t* items;
  uint32_t split_k;              // items per heavy tile (1 = no splitting; 2, 4, 8)
  int32_t split_factor;          // heavy: cost > split_factor x a resident wave's share (-1: auto)
  uint32_t split_prio;           // heavy items run at raised wave priority (s_setprio 3)
  uint32_t coop;                 // heavy tiles run cooperatively by a whole workgroup (BUNDLE_CULL_LDS)
  uint32_t plan_valid;           // tile_cost holds the previous trace's costs of this context
  uint32_t probe;                // a 1-sample planning probe (HRT_OPT_PROBE): launched as the diagnostics
                                 // instantiation (<.., true>, all diagnostics pointers null) so that
                                 // profilers list it apart from the frame's trace kernel
  uint32_t num_cus;              // compute units of the device (persistent grid size)
  // BUNDLE_BVH: bounce-segment hierarchy built by hrt_set_scene (hrt_bvh.h records); nullptr = none.
  const float4* bvh_nodes;       // 4 float4 per node, preorder with escape indices
  const float4* bvh_wq_nodes;    // 3 float4 per node: BUNDLE_WQ's image (hrt_bvh.h make_wq_nodes), or nullptr
  uint32_t bvh_wq_n_nodes;       // its nodes
  uint32_t bvh_wq_width;         // its largest group (children per node-stack entry)
  const float4* bvh_prims;       // 4 float4 per leaf triangle
  const float4* bvh_irregular;   // 4 float4 per entry outside the analysis (tested for every ray)
  const uint32_t* bvh_band_off;  // 6 bvh_dir_res^2 + 1 offsets: grazing-band prims per direction cell
  uint32_t bvh_dir_res;          // direction cells per cube-map face edge
  uint32_t bvh_sah_milli;        // hierarchy quality (HRT_SCENE_BVH_SAH_MILLI)
  const void* bvh_band;          // grazing-band entries: prim indices, 16-bit (32-bit when bvh_band_wide)
  const float4* bvh_band_nhat;   // per prim: its unit normal (the entries' pre-check)
  const uint32_t* bvh_band_rec;  // BUNDLE_WQ: 8 dwords per direction cell (start, length, 12 first entries), or null
  uint32_t bvh_band_wide;
  uint32_t bvh_band_bits;        // bit width of the longest band list
  uint32_t cam_lists_ready;      // (host) cam_tris / cam_cull / cam_meta already hold this camera's lists
  const uint32_t* bvh_entries;   // per leaf prim: triangle index | mesh << 26 (BUNDLE_BVH_LDS)
  const uint32_t* bvh_keybase;   // per mesh: key = keybase[m] + triangle index
  uint32_t bvh_n_nodes, bvh_n_irregular, bvh_n_prims, bvh_n_meshes;
  float bvh_abs_coef, bvh_rel_t;  // box-test t-slack (hrt_bvh.h)
  uint32_t bvh_max_leaf;         // largest leaf triangle count of the hierarchy
  uint32_t wq_ncap, wq_tcap;     // BUNDLE_WQ: per-wave node / triangle pair stack capacities (plan_trace)
  // Frames per launch (persistent variants, hrt_compute_n): frame f (0 <= f < n_frames) uses
  // rng_offset + f and writes img8 / img32 + f * frame_stride pixels.  0 or 1: one frame.
  uint32_t n_frames;
  size_t frame_stride;
  uint32_t bvh_node_r;  // BUNDLE_WQ: trace_bundle_wq_nr, box margins with a per-node R (HRT_OPT_WQ_NODE_RADIUS)
  float bvh_band_tau;   // the grazing band's width tau_g the hierarchy and band lists were built for
  float bvh_band_a1;    // max over prims of |a|_1: the band's plane filter tolerance (bvh_band_nhat .w = n^.a)
  uint32_t grab_always; // (debug, HRT_DEBUG_OPT_GRAB_RUNS) persistent waves take kGrab items per atomic to the end
  // (builds with -DHRT_TIMELINE=1, HRT_DEBUG_OPT_TIMELINE) per executed work item of the persistent kernels:
  // {s_memrealtime at its start, when its tile list was built, at its end, tile | log2 k << 22 | s << 25 |
  // hot << 31 | frame << 32 | run << 40 | sky << 47 | resident wave << 48}; timeline_count counts the records (capacity timeline_cap)
  unsigned long long* timeline;
  uint32_t* timeline_count;
  uint32_t timeline_cap;
  // persistent kernels (HRT_TL_PREPASS): per 8x8 tile of this launch, the wave's primary triangle list and
  // octant table as build_tile_list makes them (kTlRecWords words: list entries per lane, octant test sums
  // per lane, n, ok, aabb lo / hi, aabb_ok), filled by the tile_lists kernel before the trace; nullptr = off
  uint32_t* tl_cache;
  uint32_t tl_lists_ready;  // tl_cache already holds this camera's lists (hrt_api.cpp launch_frames): no tile_lists
  uint32_t split_factor4;   // (host side, launch_trace) the heavy threshold in quarters of a wave's share; 0: split_factor
  unsigned long long* sky_units;  // the work units (tile x frame) trace_sky has run (hrt_debug_sky_units)
  uint32_t sky_lane;        // (launch_trace) this launch's plan ends in its sky items and trace_sky runs beside the main kernel
  // BUNDLE_WQ_L2: the breadth-first node image (hrt_bvh.h make_wq_nodes_bfs; bvh_wq_n_nodes records), uploaded for
  // the contexts that select the variant, else nullptr; the HRT_OPT_WQ_LDS_NODES request (-1: auto); and the slots
  // the launch keeps in LDS (plan_trace, wq_l2_plan)
  const float4* bvh_wq_nodes_bfs;
  int32_t wq_lds_nodes_opt;
  uint32_t wq_lds_nodes;
};
// The sky lane of a trace lane (HRT_OPT_SKY_LANE): the side stream trace_sky runs on and the events a
// launch forks to it and joins it back with.
struct SkyLane {
  hipStream_t stream;
  hipEvent_t fork, join;
  bool run;  // false: the stream's first use -- an empty trace_sky launch only, so that its queue and scratch
             // exist before the first launch that forks to it (a one-time cost of tens of ms)
};
constexpr uint32_t kTlRecWords = 136;
// The plan of a tile-masked launch (hrt_refine_tiles): the persistent kernel runs only the tiles
// whose bit is set, from a plan made in buffers of the context's own -- p's sched, tile_cost and item_buf (the
// lane's) are read for the plan's input and never written.  Host side only: TraceParams is unchanged.
struct MaskedPlan {
  const uint32_t* tile_bits;  // tile t = tx + ty tiles_x is bit t & 31 of word t >> 5
  uint32_t* sched;            // kSchedWords words
  uint32_t* items;            // tiles x 64 item words
  uint32_t* cost;             // tiles words: where the launch's kernels leave their tile costs (scratch)
  uint32_t tiles_selected;    // set bits of tile_bits, > 0 (the auto split factor's tile count)
  bool costs_valid;           // p.tile_cost holds a previous trace's costs (else every selected tile costs 1)
};

// Per device, once: the dynamic-LDS limits of the persistent kernels (hipFuncSetAttribute).
hipError_t ensure_kernel_attributes(int device);
// What a launch's plan reads of p: plan_trace(plan_scene(p), variant) is the kernel an HRT_KERNEL_* request
// runs with its workgroups and LDS, plan_query(plan_scene(p), method) a query's (hrt_launch_plan.h).
PlanScene plan_scene(const TraceParams& p);
// Launches the trace kernel(s) of p's plan.
// sky: BUNDLE_WQ's product kernels run a planned launch's sky items on trace_sky beside the main kernel
// (forked from `stream` after the planner kernels, joined back into it before launch_trace returns);
// nullptr: every item runs on the main kernel.
// masked: a persistent kernel's launch over the selected tiles only (above); the tile count must fit the item word.
hipError_t launch_trace(const TraceParams& p, const LaunchPlan& plan, hipStream_t stream, const SkyLane* sky = nullptr,
                        const MaskedPlan* masked = nullptr);
// hrt_debug_tile_lists: camera_lists, then tile_lists into p.tl_cache (tiles x kTlRecWords); refine 0: the
// cap rule alone, else the product's lists (cap, then corner directions per tile and per pixel).
hipError_t launch_tile_lists(const TraceParams& p, uint32_t refine, hipStream_t stream);
// Ray centres (first + px * x) + py * y for every pixel of a width x height image (hrt_generate_rays).
hipError_t launch_make_rays(float4* rays, uint32_t width, uint32_t height, const float first[3], const float px[3],
                            const float py[3], hipStream_t stream);
hipError_t launch_tri_normals(const hrt_triangle* tris, float4* nhat, uint32_t n, hipStream_t stream);
// BUNDLE_WQ's per-cell band records from the offsets and the 16-bit lists (hrt_kernels.hip band_cell).
hipError_t launch_band_records(const uint32_t* off, const uint32_t* band16, uint32_t* rec, uint32_t cells,
                               hipStream_t stream);
// hrt_debug_math_check: fast division / sqrt paths vs the IEEE sequences (out[4] device counters).
hipError_t launch_math_check(uint32_t n, uint32_t seed, unsigned long long* out, hipStream_t stream);
hipError_t launch_band_flatten_check(const uint32_t* n, const uint32_t* b0, uint32_t rounds, uint32_t* out,
                                     hipStream_t stream);  // BandFlat on 64 given lists
hipError_t launch_math_check_rng(unsigned long long* out, hipStream_t stream);  // all 2^32 RNG states
// the pair traversal's LDS handoff protocol on a scripted wave (hrt_debug_wq_protocol)
hipError_t launch_wq_protocol_check(uint32_t rounds, const uint32_t* cnt, const uint32_t* take, const uint32_t* tgt,
                                    const unsigned long long* val, const unsigned long long* seed, uint32_t* popped,
                                    unsigned long long* seen, unsigned long long* slots, uint32_t* depth,
                                    hipStream_t stream);
// Ray queries (hrt_intersect / hrt_intersect_primary): the query kernels' own arguments,
// passed after the TraceParams block (world_hit_bounce_wq reads its constants through the kernarg
// segment's start).  One ray per lane: ray i of the launch is rays[2 i], rays[2 i + 1] (hrt_ray_query),
// or, primary, the un-jittered ray of pixel (x0 + k % w, y0 + k / w) with k = first + i; its hit goes to
// hits[2 i], hits[2 i + 1] (hrt_hit).
struct QueryArgs {
  const float4* rays;         // n hrt_ray_query records (nullptr: primary)
  float4* hits;               // n hrt_hit records
  unsigned long long* stats;  // [0] rays answered by the literal scan (non-finite), [1] triangle tests; or nullptr
  uint32_t n;                 // rays of this launch
  uint32_t first;             // primary: the rectangle index of ray 0
  uint32_t x0, y0, w;         // primary: the rectangle's corner and width
};
// Launches q.n rays as p's plan_query says; p.pc holds the sphere / mesh counts (and, primary, the camera).
hipError_t launch_query(const TraceParams& p, const QueryArgs& q, const QueryPlan& plan, bool primary, hipStream_t stream);
// Occlusion queries (hrt_occluded): any hit of q.n caller rays (q.rays; q.hits unused), ray i
// as bit i & 31 of bits[i >> 5]: ceil(q.n / 32) words, each written in full.  q.stats: [0], [1] as above,
// [2] the rays whose bit is 1; or nullptr.
hipError_t launch_occluded(const TraceParams& p, const QueryArgs& q, uint32_t* bits, const QueryPlan& plan,
                           hipStream_t stream);
// Radiance queries (hrt_radiance): the reference's main() for n caller records.  Query i
// is queries[2 i] = (origin, seed bits), queries[2 i + 1] = (centre, -) (hrt_radiance_query); its result
// (colour / num_samples, 1.0) goes to out[i] as one 16-byte store.  p.pc is the caller's push block.
struct RadianceArgs {
  const float4* queries;
  float4* out;
  unsigned long long* stats;  // [0] segments the literal scan answered (irregular), [1] segments, [2] triangle
                              // tests; or nullptr
  uint32_t* next;             // PAIRS: the launch's query counter (zero when the launch starts)
  uint32_t n;                 // queries of this launch
};
hipError_t launch_radiance(const TraceParams& p, const RadianceArgs& q, const QueryPlan& plan, hipStream_t stream);
// The first-hit pass (hrt_first_hits TILES): the un-jittered primary ray of every pixel of the
// p.pc.width x p.pc.height image, one wave per 8x8 tile from the tile's primary triangle list; pixel (x, y)'s
// hit goes to hits[2 (x + y width)], hits[2 (x + y width) + 1].  p.cam_start / cam_count / cam_tris / cam_cull
// are the pass's own camera buffers, p.pc.jitter_size the reach the lists are built for (0).
struct FirstHitsArgs {
  float4* hits;
  // [0] rays answered by the literal scan, [1] triangle tests, [2] tiles answered from their list, [3] of those
  // the empty ones of a scene without spheres, [4] fallback tiles, [5] list entries that reached the exact test;
  // nullptr: the kernel without counting code
  unsigned long long* stats;
};
constexpr uint32_t kFirstHitsStatWords = 6;
// camera_lists into p's camera buffers unless lists_ready, then first_hits_tiles
hipError_t launch_first_hits_tiles(const TraceParams& p, const FirstHitsArgs& a, bool lists_ready, hipStream_t stream);

}  // namespace hrt
