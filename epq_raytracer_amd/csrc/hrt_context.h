// hrt_context.h -- the context behind the C ABI (internal; shared by hrt_api.cpp and hrt_comm.cpp).
//
// A context owns everything the reference's RayTracePipeline + DiffusePipeline own on the Vulkan
// side (src/raytrace_pipeline.rs:31-46, src/diffuse.rs:22-30): the scene buffers, the trace image,
// the accumulated image and the queue -- plus counters, timing events and, for a row-tile partition,
// the RCCL communicator of the framebuffer gather.
//
// Streams.  `stream` (the context's stream, hrt_stream) carries every operation except the trace
// kernels of hrt_trace, which rotate over up to three trace lanes, each with its own stream, trace
// image, planner buffers and camera lists.  Frame k+1's trace does not depend on frame k's (only the
// combiner folds them, in order), so the next frame's trace starts on the CUs the current one's last
// work items leave idle (the reference's realtime loop, src/main.rs:41-57, dispatches one trace +
// combine per frame).  With three lanes frame k+2's trace waits only for frame k-1's combiner, which
// has long run, so a combiner that cannot get a CU while a persistent trace holds them all never
// stalls the next trace.  Ordering is by events only:
//   * a lane's trace waits for `lane.free` -- recorded on `stream` after the last operation that read
//     the lane's buffers (the combiner of the frame it traced before, a read_image, compute_n);
//   * an operation on `stream` that reads a lane's trace image waits for `lane.done`.
// Results are the serial loop's bytes by construction: the combiner runs in call order on one stream.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "hip_raytrace.h"

namespace hrt {

constexpr int kSkyUnitsCounter = 3 + HRT_NUM_DIAG;  // work units run by trace_sky (hrt_debug_sky_units)
constexpr int kNumCounters = 4 + HRT_NUM_DIAG;  // segments, triangle tests, wave steps, diagnostics, sky units
#ifndef HRT_LANES
#define HRT_LANES 3
#endif
constexpr int kLanes = HRT_LANES;  // trace lanes (HRT_OPT_OVERLAP uses 1..kLanes of them)

struct EventPair {
  hipEvent_t start = nullptr, stop = nullptr;
  uint32_t frames = 1;  // frames the timed launch traced
};

// Device buffers of one uploaded scene (hrt_set_scene builds a complete new set, then swaps it in).
struct SceneBufs {
  float4* rays = nullptr;
  hrt_sphere* spheres = nullptr;
  hrt_triangle* tris = nullptr;
  float4* tri_nhat = nullptr;      // normalize(tri.normal) per triangle
  hrt_mesh* meshes = nullptr;
  float4* bvh_nodes = nullptr;     // BUNDLE_BVH hierarchy (hrt_bvh.h)
  float4* bvh_wq_nodes = nullptr;  // its 48 B node image for BUNDLE_WQ (nullptr above 65535 nodes)
  // BUNDLE_WQ_L2's breadth-first image: kept on the host (at most 3 MB) and uploaded only for a context that
  // selects the variant -- by hrt_set_scene when the option is already set, else by the hrt_set_option that sets it
  float4* bvh_wq_nodes_bfs = nullptr;
  std::vector<float> wq_bfs_host;
  float4* bvh_prims = nullptr;
  float4* bvh_irregular = nullptr;
  uint32_t* bvh_band_off = nullptr;
  uint32_t* bvh_entries = nullptr;
  uint32_t* bvh_keybase = nullptr;
  void* bvh_band = nullptr;          // grazing-band entries: prim indices, 2 B (4 B when bvh_band_wide)
  float4* bvh_band_nhat = nullptr;   // per prim: n^ (the entries' pre-check)
  uint32_t* bvh_band_rec = nullptr;  // per direction cell: start, length, first 12 entries (16-bit lists only)
  uint32_t bvh_band_wide = 0;
  uint32_t bvh_band_bits = 0;        // bit width of the longest band list
  // per trace lane: compacted camera-facing records of the frame (camera_lists)
  uint32_t* cam_meta[kLanes] = {};  // cam_start[n_meshes], cam_count[n_meshes]
  float4* cam_tris[kLanes] = {};    // 64 B each
  float4* cam_cull[kLanes] = {};    // 80 B each
  uint32_t n_spheres = 0, n_tris = 0, n_meshes = 0, cam_capacity = 0;
  uint32_t bvh_info[HRT_NUM_SCENE_INFO] = {};  // hrt_get_scene_info
  float bvh_abs_coef = 0.0f, bvh_rel_t = 0.0f, bvh_band_tau = 0.0f, bvh_band_a1 = 0.0f;
  uint32_t bvh_built_leaf = 4, bvh_dir_res = 64;
  uint32_t bvh_wq_n = 0, bvh_wq_width = 2;  // BUNDLE_WQ image: nodes, largest group
};
void free_scene(hrt_context* ctx, SceneBufs& s, bool keep_rays);

// One trace lane (see the header comment).
struct Lane {
  hipStream_t stream = nullptr;
  void* trace = nullptr;  // the lane's trace image: local_rows x W pixels in the context's format
  uint32_t* sched = nullptr;      // persistent kernels' scheduler words (hrt_kernels.h)
  uint32_t* tile_cost = nullptr;  // per 8x8 tile
  uint32_t* item_buf = nullptr;   // planned work items (tiles x 64)
  uint32_t* tl_cache = nullptr;   // the persistent kernels' whole-tile lists (tiles x hrt::kTlRecWords, tile_lists)
  bool plan_valid = false;        // tile_cost describes this lane's last trace (same scene)
  // the lane's camera lists (camera_lists) hold the records of this camera position (same scene):
  // a trace from the same position skips rebuilding them
  bool cam_ready = false;
  uint32_t cam_key[4] = {};       // cam_pos bits, num_meshes
  bool tl_ready = false;          // tl_cache holds the tile lists of tl_key's camera (tile_lists ran)
  uint32_t tl_key[14] = {};       // cam_pos, mat3 of cam_alignment_mat, jitter_size bits, num_meshes
  hipEvent_t done = nullptr;      // recorded on `stream` after each trace / clear of the lane
  hipEvent_t free = nullptr;      // recorded on the context stream after the lane's last reader
  bool done_set = false, free_set = false;
  // recorded on ANOTHER context's stream after its last read of this lane's trace image
  // (hrt_accumulate_history_from with this context as the source): a second event, because `free` is
  // re-recorded by this context's own calls on its own stream, which never waits for the other's.  The
  // lane's next writer waits for both.  Created by the first such read
  hipEvent_t foreign = nullptr;
  bool foreign_set = false;
  // the lane's sky lane (HRT_OPT_SKY_LANE, hrt_kernels.h SkyLane): created by the first launch that uses it
  hipStream_t sky_stream = nullptr;
  hipEvent_t sky_fork = nullptr, sky_join = nullptr;
};

// Multi-GPU framebuffer gather (hrt_comm.cpp).
struct Comm;
void comm_release(hrt_context* ctx);

// Pinned host staging for uploads: two chunks, filled by the CPU while the DMA engine drains the other.
struct Staging {
  void* buf[2] = {};
  hipEvent_t ev[2] = {};
  bool used[2] = {};
  size_t chunk = 0;
};

}  // namespace hrt

struct hrt_context {
  int device = 0;
  hipStream_t stream = nullptr;
  uint32_t width = 0, height = 0, mode = HRT_MODE_RGBA8;
  uint32_t row_tile = 0, part_index = 0, part_count = 1, local_rows = 0;

  hrt::SceneBufs scene;
  uint32_t n_rays = 0;
  bool scene_set = false;

  hrt::Lane lane[hrt::kLanes];
  int cur_lane = 0;           // lane of the most recent trace (its image is "the trace image")
  bool lane_used = false;     // a trace / init has run since creation
  uint32_t busy_split = 2;    // HRT_OPT_BUSY_SPLIT: grid share of a trace launched while another runs
  uint32_t overlap = hrt::kLanes;  // HRT_OPT_OVERLAP: trace lanes in rotation (1: every trace on lane 0)

  void* accum = nullptr;    // the accumulated image: local_rows x W pixels in the context's format
  void* scratch = nullptr;  // format conversion for hrt_read_image
  unsigned long long* counters = nullptr;
  unsigned long long* tile_cycles = nullptr;  // diagnostics: shader clocks per 8x8 tile of the last trace
  uint32_t split_k = 0, split_prio = 1;  // split 0: auto (per kernel, hrt_launch_plan.h)
  int32_t split_factor = -1;  // auto
  uint32_t grid_cus = 0;  // HRT_OPT_GRID_CUS (debug build; 0: every CU)
  uint32_t coop = 1;      // HRT_OPT_COOP
  uint32_t wq_node_cap = 0;  // HRT_OPT_WQ_NODE_CAP (0 = auto)
  uint32_t probe = 1;        // HRT_OPT_PROBE
  uint32_t frames_per_launch = 64;  // HRT_OPT_FRAMES_PER_LAUNCH (hrt_compute_n)
  void* frame_stack = nullptr;      // hrt_compute_n: frame_stack_frames trace images
  uint32_t frame_stack_frames = 0;
  uint32_t frame_stack_failed = 0;  // a whole-launch stack of this many frames did not fit: not retried
  uint32_t num_cus = 0;
  uint32_t bvh_leaf = 0;  // HRT_OPT_BVH_LEAF_SIZE for the next hrt_set_scene (0 = auto, hrt_bvh.h)
  uint32_t wq_node_radius = 0;  // HRT_OPT_WQ_NODE_RADIUS (0 = auto)
  int32_t wq_lds_nodes = -1;    // HRT_OPT_WQ_LDS_NODES (-1 = auto)
  int32_t sky_lane = -1;        // HRT_OPT_SKY_LANE (-1 = auto)
  uint32_t bvh_width = 4;  // HRT_OPT_BVH_WIDTH (hrt_bvh.h kWqDefaultWidth) for the next hrt_set_scene
  int64_t debug_fail_alloc = 0;   // debug build: fail the n-th device allocation of the next hrt_set_scene
  uint32_t debug_grab_runs = 0;   // debug build: HRT_DEBUG_OPT_GRAB_RUNS
  int64_t debug_stack_limit = 0;  // debug build: HRT_DEBUG_OPT_STACK_LIMIT (frame-stack bytes that fit)
  uint32_t debug_wq_tri_cap = 0;  // debug build: HRT_DEBUG_OPT_WQ_TRI_CAP (triangle-pair stack capacity)
  unsigned long long* timeline = nullptr;  // HRT_TIMELINE builds: HRT_DEBUG_OPT_TIMELINE records (4 u64 each)
  uint32_t* timeline_count = nullptr;
  uint32_t timeline_cap = 0;

  int variant = 0;
  bool counters_on = true;
  bool diag_on = false;
  uint32_t sec_batch = 0;  // HRT_OPT_SECONDARY_BATCH (0 = auto per kernel, hrt_launch_plan.h)
  uint32_t prim_batch = 0;  // HRT_OPT_PRIMARY_BATCH (0 = auto per kernel, hrt_launch_plan.h)
  int last_kernel = 0, last_block = 0;  // what the last hrt_trace launched (hrt_stats)
  uint32_t last_frames = 0;             // ... and the frames that launch held

  struct Import {
    hipExternalMemory_t mem;
    void* ptr;
    uint64_t bytes;  // mapped size (hrt_present accepts a target inside [ptr, ptr + bytes))
  };
  std::vector<Import> imports;           // hrt_import_external_memory (released by hrt_destroy)
  // Present tickets (hrt_present): ticket t's event is present_ev[(t - 1) % kPresentRing], recorded on
  // `stream` after the pass; present_issued = the newest ticket.  Events are created on first use.
  static constexpr uint32_t kPresentRing = 8;
  hipEvent_t present_ev[kPresentRing] = {};
  uint64_t present_issued = 0;
  std::vector<hrt::EventPair> event_pool;  // reusable
  std::vector<hrt::EventPair> pending;     // recorded, not yet harvested (a ring of kMaxPending)
  uint64_t traces = 0, accumulates = 0;
  float last_ms = 0.0f, total_ms = 0.0f;

  struct Guard {
    void* ptr;
    size_t bytes;
  };
  std::vector<Guard> guards;  // debug build: guarded device allocations (hrt_debug_check_guards)
  hrt::Staging staging;
  // Deferred combiner (HRT_OPT_DEFER_COMBINE).  The accumulator is observable only through
  // hrt_read_image / hrt_stream / hrt_synchronize, so hrt_accumulate after an hrt_trace only records
  // (ring slot, frame): the trace wrote a slot of a ring of frame images instead of its lane's image,
  // and the recorded frames are folded in frame order (fold_frames, the hrt_compute_n combiner)
  // at the next observation or when the ring is full -- the per-frame combine's bytes, without a
  // combiner kernel queued between every two traces.
  void* ring = nullptr;        // ring_n frame images (context format), allocated by the first trace
  uint32_t ring_n = 0, ring_next = 0;
  int cur_slot = -1;           // ring slot of the most recent trace (-1: its lane's own image)
  struct Pend {
    uint32_t slot, frame;
  };
  std::vector<Pend> pend;      // recorded, not yet folded (consecutive slots and frames)
  hipEvent_t fold_done = nullptr;  // recorded on `stream` after the last fold (a slot's next trace waits)
  bool fold_set = false;
  // fold_done's counterpart for a reader on another context's stream (Lane::foreign): recorded there after
  // hrt_accumulate_history_from has read a ring slot of this context; a slot's next trace waits for both
  hipEvent_t fold_foreign = nullptr;
  bool fold_foreign_set = false;
  uint32_t defer = 0;          // HRT_OPT_DEFER_COMBINE (off: measured slower, hip_raytrace.h)
  // Fold records (HRT_OPT_FOLD_RECORDS, hrt_compute_until).  Record t (0-based since the option was set)
  // lives in fold_ring[t % HRT_FOLD_RECORD_RING]: the host zeroes the slot on `stream` before the fold
  // that adds its counts and keeps the slot's frame number in fold_frame.  fold_scratch is the ring of
  // hrt_compute_until's count pass (slot f = frame f of the launch).  Both are allocated on first use.
  hrt_fold_record* fold_ring = nullptr;
  hrt_fold_record* fold_scratch = nullptr;
  std::vector<uint32_t> fold_frame;
  uint64_t fold_total = 0;
  uint32_t fold_on = 0;
  // Ray queries (hrt_intersect / hrt_intersect_primary): staging for host-side rays and hits (kQueryChunk
  // records each) and the two statistics words, allocated by the first query
  void* query_rays = nullptr;
  void* query_hits = nullptr;
  unsigned long long* query_stats = nullptr;
  // Occlusion queries (hrt_occluded): staging for a chunk's bits (kQueryChunk / 32 words) when the caller's
  // are host memory, and the three statistics words
  void* occl_bits = nullptr;
  unsigned long long* occl_stats = nullptr;
  // Radiance queries (hrt_radiance): staging for a chunk's results (kQueryChunk x 16 bytes) when the caller's
  // are host memory, and four words: the three statistics counts, then the PAIRS kernel's query counter
  void* rad_out = nullptr;
  unsigned long long* rad_words = nullptr;
  // The denoise pass (hrt_denoise, hrt_denoise_present): the two float4 images its passes ping-pong between,
  // allocated by the first call, and the compact guide ({n, t} and the surface key per pixel), by the first
  // guided one
  void* dn_img[2] = {};
  void* dn_guide = nullptr;
  void* dn_keys = nullptr;
  // Temporal history (hrt_reproject, hrt_accumulate_history, hrt_fill_history, hrt_read_history): the count
  // image N, one uint32 per pixel, allocated and zeroed by the first call of any of the four; and what
  // hrt_reproject writes A' and N' into, allocated by its first call -- after the pass they are swapped with
  // `accum` and `hist_cnt`, so the pass never reads a texel it has replaced
  uint32_t* hist_cnt = nullptr;
  uint32_t* hist_cnt_next = nullptr;
  void* hist_accum_next = nullptr;
  // The variance-guided denoise (hrt_accumulate_history_moments, hrt_reproject_moments, hrt_fill_moments,
  // hrt_read_moments, hrt_denoise_variance[_present]): the moments image M, two floats per pixel, allocated and
  // zeroed by the first call of any of them; what hrt_reproject_moments writes M' into, swapped with hist_mom after
  // the pass; and the staging of a variance_dst in host memory (one float per pixel).  The filter's passes run
  // between dn_img[0] and dn_img[1], with dn_guide and dn_keys
  float* hist_mom = nullptr;
  float* hist_mom_next = nullptr;
  float* var_stage = nullptr;
  // Object motion (hrt_reproject_motion[_moments]): the staging ring of the callers' tables.  A call copies its
  // tables into slot motion_next's pinned buffer, enqueues the copy to the slot's device buffer and the pass on
  // `stream`, and records the slot's event after the pass: the slot's next user waits for that event on the host
  // before it writes the pinned buffer, so neither buffer is reused while a copy or a pass that reads it is in
  // flight.  Buffers and events are made by the first call that needs them and grown for a larger table
  struct MotionSlot {
    void* host = nullptr;
    void* dev = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool used = false;
  };
  MotionSlot motion_ring[HRT_MOTION_RING];
  uint32_t motion_next = 0;
  // Guided upsampling (hrt_upsample, hrt_upsample_present, hrt_order_after): the staging image of a result that
  // goes to host memory (up_stage_bytes of it, grown when a larger result comes), and the event hrt_order_after
  // records on this context's stream when it is the producer.  Each is made by the first call that needs it
  void* up_stage = nullptr;
  size_t up_stage_bytes = 0;
  hipEvent_t order_ev = nullptr;
  // The adaptive refinement (hrt_refine_select, hrt_refine, hrt_refine_until): the mask's staging (one bit per pixel)
  // for a mask in host memory and for hrt_refine_until's own; the compact lists of a QUERIES pass (npix entries:
  // hrt_radiance_query records, pixel indices, results); and two 64-bit words: the selected count, then the
  // list's entry counter.  Each is allocated by the first call that needs it
  uint32_t* rf_mask = nullptr;
  void* rf_queries = nullptr;
  uint32_t* rf_index = nullptr;
  void* rf_rgba = nullptr;
  unsigned long long* rf_words = nullptr;
  // The tile-masked refinement (hrt_refine_tiles): one bit per 8x8 tile, three 64-bit counts (selected pixels,
  // selected tiles, their real pixels), and the masked launches' own plan -- sched words, item list and a scratch
  // cost image, so that lane 0's are never written.  Allocated by the first call, freed by hrt_destroy
  uint32_t* rt_bits = nullptr;
  unsigned long long* rt_counts = nullptr;
  uint32_t* rt_sched = nullptr;
  uint32_t* rt_items = nullptr;
  uint32_t* rt_cost = nullptr;
  // The first-hit pass (hrt_first_hits): its own camera buffers (a fourth set beside the lanes', the scene's
  // sizes), allocated by the first TILES call and dropped by hrt_set_scene; fh_key = the camera position's bits
  // and num_meshes the records were built for (fh_ready: by a launch already enqueued on `stream`); the device
  // record a counted call adds to (hrt::kFirstHitsStatWords words) and what the host knows of that call
  uint32_t* fh_cam_meta = nullptr;
  float4* fh_cam_tris = nullptr;
  float4* fh_cam_cull = nullptr;
  bool fh_ready = false;
  uint32_t fh_key[4] = {};
  unsigned long long* fh_stats = nullptr;
  uint32_t fh_counted_method = 0, fh_counted_tiles = 0;  // method 0: no counted call yet
  hrt::Comm* comm = nullptr;  // hrt_comm_init / hrt_comm_init_all
  uint32_t comm_timeout_ms = 120000;  // HRT_OPT_COMM_TIMEOUT_MS (0: wait forever)

  std::string err;

  size_t npix() const { return (size_t)local_rows * width; }
  // the pixels of the local rows whose global row is below height: a prefix of the local rows (the padding
  // rows of a row-tile part follow them) -- what a fold record counts
  size_t real_pix() const {
    if (part_count <= 1) return npix();
    uint32_t rows = 0;
    for (uint32_t r = 0; r < local_rows; ++r)
      if (((uint64_t)(r / row_tile) * part_count + part_index) * row_tile + r % row_tile < height) ++rows;
    return (size_t)rows * width;
  }
  bool f32() const { return mode != HRT_MODE_RGBA8; }  // the format of every image of the context (hrt_image.h)
  size_t px_bytes() const { return f32() ? 16 : 4; }
  size_t num_tiles() const { return (size_t)((width + 7) / 8) * ((local_rows + 7) / 8); }
};

namespace hrt {

hrt_status fail(hrt_context* ctx, hrt_status st, const std::string& msg);
hrt_status hip_fail(hrt_context* ctx, hipError_t e, const char* what);
hrt_status bind(hrt_context* ctx);               // make the context's device current
hipError_t dev_alloc(hrt_context* ctx, void** p, size_t bytes);  // guarded in the debug build
void dev_free(hrt_context* ctx, void* p);
hrt_status join_lanes(hrt_context* ctx);         // the context stream waits for every lane's trace
hrt_status wait_lane(hrt_context* ctx, int l);   // ... for lane l's trace
hrt_status release_lane(hrt_context* ctx, int l);  // lane l's buffers are free after the stream's work so far
// Reads image_id of this context's local rows in its own pixel format, ordered on ctx->stream (the
// accumulator after every deferred combine has been folded).
const void* local_image(hrt_context* ctx, uint32_t image_id);
// Folds the deferred combines (hrt_context::pend) into the accumulator on ctx->stream.
hrt_status flush_combines(hrt_context* ctx);
// dst <- npix pixels at src (context format) converted to fmt via scratch, ordered on ctx->stream; blocking.
hrt_status copy_frame_out(hrt_context* ctx, const void* src, size_t npix, uint32_t fmt, void* dst, void* scratch);
// hrt_read_image on a context with a communicator (hrt_comm.cpp); arg = the caller's own argument
// check, agreed on by every rank of a process communicator before any of them gathers.
hrt_status comm_read_image(hrt_context* ctx, uint32_t image_id, uint32_t fmt, void* dst, size_t bytes,
                           hrt_status arg);
// The gathered present (hrt_present / hrt_accumulate_present on a context with a communicator, hrt_comm.cpp).
struct PresentTarget;  // hrt_image.h
// HRT_OK when ctx is member 0 of an intact hrt_comm_init_all group; else HRT_ERR_INVALID_ARGUMENT with
// the reason (`who` prefixes the message).  Host only: nothing is enqueued.
hrt_status comm_present_check(hrt_context* ctx, const char* who);
// The members of ctx's hrt_comm_init_all group in part order (nullptr: no such group).
const std::vector<hrt_context*>* comm_group_members(const hrt_context* ctx);
// Enqueues the gather of image_id to the root and the fused present kernel on the root's stream, with no
// host wait (the caller has run comm_present_check and issues the ticket on root->stream afterwards).
// image_id: HRT_IMG_TRACE or HRT_IMG_ACCUM.  Leaves the root's device current.
hrt_status comm_present(hrt_context* root, uint32_t image_id, const PresentTarget& target);

}  // namespace hrt

#define HRT_HIP(ctx, call)                                        \
  do {                                                            \
    hipError_t e_ = (call);                                       \
    if (e_ != hipSuccess) return ::hrt::hip_fail((ctx), e_, #call); \
  } while (0)
