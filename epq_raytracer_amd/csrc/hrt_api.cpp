// hrt_api.cpp -- the C ABI of libhip_raytrace.so (include/hip_raytrace.h).
//
// The context (hrt_context.h) owns everything the reference's RayTracePipeline + DiffusePipeline own
// on the Vulkan side (src/raytrace_pipeline.rs:31-46, src/diffuse.rs:22-30).  Memory is allocated by
// hrt_create, hrt_set_scene and hrt_set_option; hrt_trace and hrt_accumulate only enqueue work (no
// allocation) and block only when kMaxPending timed traces are still outstanding.  hrt_compute_n
// allocates its frame images on first use.
//
// Built twice: libhip_raytrace.so (production) and, with -DHRT_DEBUG_OPTIONS, libhip_raytrace_debug.so,
// which also accepts the diagnostics-only options (HRT_OPT_PRIORITY = 2, HRT_OPT_GRID_CUS,
// HRT_DEBUG_OPT_FAIL_ALLOC, HRT_DEBUG_OPT_WQ_TRI_CAP) that leave frames incomplete, inject failures or
// force rare paths.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "hip_raytrace.h"
#include "hrt_bvh.h"
#include "hrt_context.h"
#include "hrt_denoise.h"
#include "hrt_history.h"
#include "hrt_upsample.h"
#include "hrt_resolve.h"
#include "hrt_resolve_map.h"
#include "hrt_variance.h"
#include "hrt_refine.h"
#include "hrt_host.h"
#include "hrt_image.h"
#include "hrt_kernels.h"

// (the record, push-block, hrt_create_info / hrt_layout / hrt_stats sizes and offsets are
// static_asserted by include/hip_raytrace.h itself, for every translation unit that includes it)
static_assert(sizeof(hrt_stats) == 64, "hrt_stats: ABI 4");

namespace {

thread_local std::string g_create_error;
constexpr size_t kMaxPending = 256;              // timed traces held before the oldest is harvested
constexpr size_t kStagingChunk = (size_t)8 << 20;  // pinned upload chunk (two of them)

template <typename T>
void free_dev(hrt_context* ctx, T*& p) {
  hrt::dev_free(ctx, (void*)p);
  p = nullptr;
}

// Folds the oldest timed trace into the stats (blocks until it has finished).
hrt_status harvest_one(hrt_context* ctx) {
  hrt::EventPair ev = ctx->pending.front();
  ctx->pending.erase(ctx->pending.begin());
  ctx->event_pool.push_back(ev);
  HRT_HIP(ctx, hipEventSynchronize(ev.stop));
  float ms = 0.0f;
  HRT_HIP(ctx, hipEventElapsedTime(&ms, ev.start, ev.stop));
  ctx->last_ms = ms / (float)ev.frames;  // per frame
  ctx->total_ms += ms;
  return HRT_OK;
}

hrt_status harvest_events(hrt_context* ctx) {
  while (!ctx->pending.empty()) {
    hrt_status st = harvest_one(ctx);
    if (st != HRT_OK) return st;
  }
  return HRT_OK;
}

// Every stream of the context drained.
hrt_status sync_all(hrt_context* ctx) {
  for (auto& l : ctx->lane)
    if (l.stream) HRT_HIP(ctx, hipStreamSynchronize(l.stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HRT_OK;
}

}  // namespace

namespace hrt {

hrt_status fail(hrt_context* ctx, hrt_status st, const std::string& msg) {
  if (ctx)
    ctx->err = msg;
  else
    g_create_error = msg;
  return st;
}

hrt_status hip_fail(hrt_context* ctx, hipError_t e, const char* what) {
  std::string msg = std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")";
  return fail(ctx, e == hipErrorOutOfMemory ? HRT_ERR_OUT_OF_MEMORY : HRT_ERR_HIP, msg);
}

hrt_status bind(hrt_context* ctx) {
  HRT_HIP(ctx, hipSetDevice(ctx->device));
  return HRT_OK;
}

hrt_status wait_lane(hrt_context* ctx, int l) {
  if (ctx->lane[l].done_set) HRT_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->lane[l].done, 0));
  return HRT_OK;
}

hrt_status join_lanes(hrt_context* ctx) {
  for (int l = 0; l < kLanes; ++l) {
    hrt_status st = wait_lane(ctx, l);
    if (st != HRT_OK) return st;
  }
  return HRT_OK;
}

hrt_status release_lane(hrt_context* ctx, int l) {
  HRT_HIP(ctx, hipEventRecord(ctx->lane[l].free, ctx->stream));
  ctx->lane[l].free_set = true;
  return HRT_OK;
}

// Device allocations.  The debug build surrounds every allocation with kGuardBytes of a fixed
// pattern on each side (hrt_debug_check_guards verifies them: a kernel writing past a buffer's end
// or before its start shows up there).
#ifdef HRT_DEBUG_OPTIONS
constexpr size_t kGuardBytes = 4096;
constexpr int kGuardByte = 0xA5;
#endif

hipError_t dev_alloc(hrt_context* ctx, void** p, size_t bytes) {
#ifdef HRT_DEBUG_OPTIONS
  char* base = nullptr;
  hipError_t e = hipMalloc((void**)&base, bytes + 2 * kGuardBytes);
  if (e != hipSuccess) {
    *p = nullptr;
    return e;
  }
  if ((e = hipMemset(base, kGuardByte, kGuardBytes)) != hipSuccess ||
      (e = hipMemset(base + kGuardBytes + bytes, kGuardByte, kGuardBytes)) != hipSuccess) {
    (void)hipFree(base);
    *p = nullptr;
    return e;
  }
  *p = base + kGuardBytes;
  ctx->guards.push_back({*p, bytes});
  return hipSuccess;
#else
  (void)ctx;
  return hipMalloc(p, bytes);
#endif
}

void dev_free(hrt_context* ctx, void* p) {
  if (!p) return;
#ifdef HRT_DEBUG_OPTIONS
  for (size_t i = 0; i < ctx->guards.size(); ++i)
    if (ctx->guards[i].ptr == p) {
      ctx->guards.erase(ctx->guards.begin() + (long)i);
      (void)hipFree(static_cast<char*>(p) - kGuardBytes);
      return;
    }
#else
  (void)ctx;
#endif
  (void)hipFree(p);
}

// The trace image: the most recent trace's ring slot, or its lane's own image.
void* trace_image(hrt_context* ctx) {
  if (ctx->cur_slot >= 0) return static_cast<char*>(ctx->ring) + (size_t)ctx->cur_slot * ctx->npix() * ctx->px_bytes();
  return ctx->lane[ctx->cur_lane].trace;
}

const void* local_image(hrt_context* ctx, uint32_t image_id) {
  if (image_id == HRT_IMG_ACCUM) {
    if (flush_combines(ctx) != HRT_OK) return nullptr;
    return ctx->accum;
  }
  if (wait_lane(ctx, ctx->cur_lane) != HRT_OK) return nullptr;
  return trace_image(ctx);
}

// HRT_OPT_FOLD_RECORDS = 1: the fold of nf frames (image f of the stack = frame frame0 + f) into the
// accumulator by the recording kernel, appending nf records to the ring -- the slots zeroed on the stream
// first, their frame numbers kept on the host.  A fold may wrap the ring's end.
static hrt_status fold_recorded(hrt_context* ctx, const void* stack, uint32_t nf, uint32_t frame0) {
  const size_t np = ctx->npix(), fb = np * ctx->px_bytes();
  const uint32_t ring = HRT_FOLD_RECORD_RING;
  for (uint32_t done = 0; done < nf;) {  // (a launch's frames have a slot each)
    const uint32_t n = std::min(nf - done, ring), slot0 = (uint32_t)(ctx->fold_total % ring);
    const uint32_t head = std::min(n, ring - slot0);
    HRT_HIP(ctx, hipMemsetAsync(ctx->fold_ring + slot0, 0, (size_t)head * sizeof(hrt_fold_record), ctx->stream));
    if (n > head)
      HRT_HIP(ctx, hipMemsetAsync(ctx->fold_ring, 0, (size_t)(n - head) * sizeof(hrt_fold_record), ctx->stream));
    for (uint32_t f = 0; f < n; ++f) ctx->fold_frame[(slot0 + f) % ring] = frame0 + done + f;
    const char* base = static_cast<const char*>(stack) + (size_t)done * fb;
    HRT_HIP(ctx, launch_fold_records(ctx->accum, base, ctx->f32(), np, ctx->real_pix(), n, frame0 + done, true,
                                     ctx->fold_ring, slot0, ctx->num_cus, ctx->stream));
    ctx->fold_total += n;
    done += n;
  }
  return HRT_OK;
}

// Every fold into the accumulator, on ctx->stream: the nf frames of a stack (image f = frame frame0 + f) by the
// recording kernel when HRT_OPT_FOLD_RECORDS is on, else one frame by the single-frame combiner (the
// realtime loop's) and several by the stack combiner.
static hrt_status fold_frames(hrt_context* ctx, const void* stack, uint32_t nf, uint32_t frame0) {
  if (ctx->fold_on) return fold_recorded(ctx, stack, nf, frame0);
  if (nf == 1)
    HRT_HIP(ctx, launch_accumulate(ctx->accum, stack, ctx->f32(), ctx->npix(), frame0, ctx->stream));
  else
    HRT_HIP(ctx, launch_accumulate_frames(ctx->accum, stack, ctx->f32(), ctx->npix(), nf, frame0, ctx->stream));
  return HRT_OK;
}

hrt_status flush_combines(hrt_context* ctx) {
  if (ctx->pend.empty()) return HRT_OK;
  // the folds read slots that traces on every lane wrote: after each lane's latest trace
  hrt_status st = join_lanes(ctx);
  if (st != HRT_OK) return st;
  const size_t fb = ctx->npix() * ctx->px_bytes();
  for (size_t i = 0; i < ctx->pend.size();) {
    size_t j = i;  // a run of consecutive slots (no wrap) and frames: one pass over the stack
    while (j + 1 < ctx->pend.size() && ctx->pend[j + 1].slot == ctx->pend[j].slot + 1 &&
           ctx->pend[j + 1].frame == ctx->pend[j].frame + 1)
      ++j;
    const char* base = static_cast<const char*>(ctx->ring) + (size_t)ctx->pend[i].slot * fb;
    if ((st = fold_frames(ctx, base, (uint32_t)(j - i + 1), ctx->pend[i].frame)) != HRT_OK) return st;
    i = j + 1;
  }
  ctx->pend.clear();
  HRT_HIP(ctx, hipEventRecord(ctx->fold_done, ctx->stream));
  ctx->fold_set = true;
  return HRT_OK;
}

void free_scene(hrt_context* ctx, SceneBufs& s, bool keep_rays) {
  if (!keep_rays) free_dev(ctx, s.rays);
  free_dev(ctx, s.spheres);
  free_dev(ctx, s.tris);
  free_dev(ctx, s.tri_nhat);
  free_dev(ctx, s.meshes);
  free_dev(ctx, s.bvh_nodes);
  free_dev(ctx, s.bvh_wq_nodes);
  free_dev(ctx, s.bvh_wq_nodes_bfs);
  free_dev(ctx, s.bvh_prims);
  free_dev(ctx, s.bvh_irregular);
  free_dev(ctx, s.bvh_band_off);
  free_dev(ctx, s.bvh_band);
  free_dev(ctx, s.bvh_band_nhat);
  free_dev(ctx, s.bvh_band_rec);
  free_dev(ctx, s.bvh_entries);
  free_dev(ctx, s.bvh_keybase);
  for (int l = 0; l < kLanes; ++l) {
    free_dev(ctx, s.cam_meta[l]);
    free_dev(ctx, s.cam_tris[l]);
    free_dev(ctx, s.cam_cull[l]);
  }
}

}  // namespace hrt

using hrt::fail;
using hrt::hip_fail;
using hrt::bind;

extern "C" uint32_t hrt_abi_version(void) { return HRT_ABI_VERSION; }

// Host only: BUNDLE_WQ_L2's LDS plan (hrt_launch_plan.h wq_l2_plan) with no stack-capacity requests.
extern "C" void hrt_debug_wq_l2_plan(uint32_t n_nodes, uint32_t width, uint32_t max_leaf, int64_t lds_nodes,
                                     uint32_t out[4]) {
  hrt::wq_l2_plan(n_nodes, width, max_leaf, lds_nodes, 0u, 0u, out);
}

extern "C" hrt_status hrt_debug_check_guards(hrt_context* ctx, uint32_t* buffers, uint32_t* corrupted) {
  if (!ctx || !buffers || !corrupted) return HRT_ERR_INVALID_ARGUMENT;
  *buffers = *corrupted = 0;
#ifdef HRT_DEBUG_OPTIONS
  hrt_status st = hrt_synchronize(ctx);
  if (st != HRT_OK) return st;
  std::vector<unsigned char> g(hrt::kGuardBytes);
  for (const auto& r : ctx->guards) {
    bool bad = false;
    for (int side = 0; side < 2 && !bad; ++side) {
      const char* at = side == 0 ? static_cast<const char*>(r.ptr) - hrt::kGuardBytes : static_cast<const char*>(r.ptr) + r.bytes;
      HRT_HIP(ctx, hipMemcpy(g.data(), at, g.size(), hipMemcpyDeviceToHost));
      for (unsigned char b : g) bad |= b != hrt::kGuardByte;
    }
    ++*buffers;
    *corrupted += bad ? 1u : 0u;
  }
  return HRT_OK;
#else
  return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_debug_check_guards: only libhip_raytrace_debug.so guards buffers");
#endif
}

// Tuning support: lane 0's per-tile costs as the last persistent launch on it recorded them (the next
// launch's plan input; shader clocks / 16 per 8x8 tile, summed over the launch's frames).
extern "C" hrt_status hrt_debug_tile_costs(hrt_context* ctx, uint32_t* out, uint32_t count) {
  if (!ctx || !out) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = hrt_synchronize(ctx);
  if (st != HRT_OK) return st;
  if (!ctx->lane[0].tile_cost) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_debug_tile_costs: no trace yet");
  const uint32_t n = std::min(count, (uint32_t)ctx->num_tiles());
  HRT_HIP(ctx, hipMemcpy(out, ctx->lane[0].tile_cost, (size_t)n * 4, hipMemcpyDeviceToHost));
  return HRT_OK;
}

// Test support: the work units (tile x frame) that trace_sky has run on this context since creation or
// hrt_reset_stats -- a test of the sky lane proves with it that the side kernel rendered items.
extern "C" hrt_status hrt_debug_sky_units(hrt_context* ctx, uint64_t* out) {
  if (!ctx || !out) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = hrt_synchronize(ctx);
  if (st != HRT_OK) return st;
  unsigned long long v = 0;
  HRT_HIP(ctx, hipMemcpy(&v, ctx->counters + hrt::kSkyUnitsCounter, sizeof v, hipMemcpyDeviceToHost));
  *out = v;
  return HRT_OK;
}

// Test support: the context's grazing-band structure as the device holds it -- the per-cell records
// (band_records), the offsets and the entry words -- so a test can hold the device-built records to the
// lists they summarise.  info = {cells, entries, wide (32-bit entries), records present}.
extern "C" hrt_status hrt_debug_band_records(hrt_context* ctx, uint32_t* rec, uint64_t rec_words, uint32_t* off,
                                             uint64_t off_words, uint32_t* list_words, uint64_t list_cap,
                                             uint32_t info[4]) {
  if (!ctx || !info) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = hrt_synchronize(ctx);
  if (st != HRT_OK) return st;
  const hrt::SceneBufs& s = ctx->scene;
  const uint64_t cells = s.bvh_band_off ? 6ull * s.bvh_dir_res * s.bvh_dir_res : 0ull;
  const uint64_t entries = s.bvh_info[HRT_SCENE_BVH_BAND_ENTRIES];
  const uint64_t words = s.bvh_band_wide ? entries : (entries + 1) / 2;
  info[0] = (uint32_t)cells;
  info[1] = (uint32_t)entries;
  info[2] = s.bvh_band_wide;
  info[3] = s.bvh_band_rec ? 1u : 0u;
  if (rec && s.bvh_band_rec && rec_words >= cells * 8)
    HRT_HIP(ctx, hipMemcpy(rec, s.bvh_band_rec, cells * 32, hipMemcpyDeviceToHost));
  if (off && s.bvh_band_off && off_words >= cells + 1)
    HRT_HIP(ctx, hipMemcpy(off, s.bvh_band_off, (cells + 1) * 4, hipMemcpyDeviceToHost));
  if (list_words && s.bvh_band && list_cap >= words && words)
    HRT_HIP(ctx, hipMemcpy(list_words, s.bvh_band, words * 4, hipMemcpyDeviceToHost));
  return HRT_OK;
}

#ifndef HRT_BUILD_ID
#define HRT_BUILD_ID "unknown"
#endif
extern "C" const char* hrt_build_id(void) { return HRT_BUILD_ID; }

extern "C" uint32_t hrt_debug_build(void) {
#ifdef HRT_DEBUG_OPTIONS
  return 1u;
#else
  return 0u;
#endif
}

extern "C" hrt_status hrt_create(const hrt_create_info* info, hrt_context** out_ctx) {
  g_create_error.clear();
  if (!info || !out_ctx) return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_create: null argument");
  *out_ctx = nullptr;
  if (info->mode != HRT_MODE_RGBA8 && info->mode != HRT_MODE_RGBA32F)
    return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_create: unknown mode");
  if (info->width == 0 || info->height == 0)
    return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_create: zero image size");
  if ((uint64_t)info->width * info->height > (1ull << 31))
    return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_create: image larger than 2^31 pixels");
  const uint32_t parts = info->part_count == 0 ? 1 : info->part_count;
  if (parts > 1 && (info->row_tile == 0 || info->part_index >= parts))
    return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_create: bad row-tile partition");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, HRT_ERR_NO_DEVICE, "hrt_create: no HIP device visible");
  int dev = info->device;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  }
  if (dev >= ndev) return fail(nullptr, HRT_ERR_NO_DEVICE, "hrt_create: device ordinal out of range");

  auto* ctx = new hrt_context();
  ctx->device = dev;
  ctx->width = info->width;
  ctx->height = info->height;
  ctx->mode = info->mode;
  ctx->part_count = parts;
  if (parts > 1) {
    ctx->row_tile = info->row_tile;
    ctx->part_index = info->part_index;
    const uint32_t tiles = (info->height + info->row_tile - 1) / info->row_tile;
    const uint32_t tiles_per_part = (tiles + parts - 1) / parts;
    ctx->local_rows = tiles_per_part * info->row_tile;
  } else {
    ctx->row_tile = info->height;
    ctx->part_index = 0;
    ctx->local_rows = info->height;
  }

  auto bail = [&](hrt_status st) {
    std::string msg = ctx->err;
    hrt_destroy(ctx);
    return fail(nullptr, st, msg);
  };
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return bail(st);
  hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e != hipSuccess) return bail(hip_fail(ctx, e, "hipStreamCreate"));
  if ((e = hrt::ensure_kernel_attributes(ctx->device)) != hipSuccess)
    return bail(hip_fail(ctx, e, "hipFuncSetAttribute(dynamic LDS)"));
  const size_t np = ctx->npix(), tiles = std::max<size_t>(ctx->num_tiles(), 1);
  for (auto& l : ctx->lane) {
    if ((e = hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking)) != hipSuccess)
      return bail(hip_fail(ctx, e, "hipStreamCreate(lane)"));
    if ((e = hipEventCreateWithFlags(&l.done, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&l.free, hipEventDisableTiming)) != hipSuccess)
      return bail(hip_fail(ctx, e, "hipEventCreate(lane)"));
    if ((e = hrt::dev_alloc(ctx, &l.trace, np * ctx->px_bytes())) != hipSuccess)
      return bail(hip_fail(ctx, e, "hipMalloc(trace)"));
    if ((e = hrt::dev_alloc(ctx, (void**)&l.sched, hrt::kSchedWords * 4)) != hipSuccess) return bail(hip_fail(ctx, e, "hipMalloc(sched)"));
    if ((e = hrt::dev_alloc(ctx, (void**)&l.tile_cost, tiles * 4)) != hipSuccess)
      return bail(hip_fail(ctx, e, "hipMalloc(tile costs)"));
    if ((e = hrt::dev_alloc(ctx, (void**)&l.item_buf, tiles * 64 * 4)) != hipSuccess)
      return bail(hip_fail(ctx, e, "hipMalloc(items)"));
    if ((e = hrt::dev_alloc(ctx, (void**)&l.tl_cache, tiles * hrt::kTlRecWords * 4)) != hipSuccess)
      return bail(hip_fail(ctx, e, "hipMalloc(tile lists)"));
  }
  if ((e = hrt::dev_alloc(ctx, &ctx->accum, np * ctx->px_bytes())) != hipSuccess)
    return bail(hip_fail(ctx, e, "hipMalloc(accum)"));
  if ((e = hrt::dev_alloc(ctx, (void**)&ctx->scratch, np * 16)) != hipSuccess) return bail(hip_fail(ctx, e, "hipMalloc(scratch)"));
  if ((e = hipEventCreateWithFlags(&ctx->fold_done, hipEventDisableTiming)) != hipSuccess)
    return bail(hip_fail(ctx, e, "hipEventCreate(fold)"));
  if ((e = hrt::dev_alloc(ctx, (void**)&ctx->counters, hrt::kNumCounters * sizeof(unsigned long long))) != hipSuccess)
    return bail(hip_fail(ctx, e, "hipMalloc(counters)"));
  {
    int cus = 0;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device)) != hipSuccess)
      return bail(hip_fail(ctx, e, "hipDeviceGetAttribute(CUs)"));
    ctx->num_cus = cus > 0 ? (uint32_t)cus : 1u;
  }
  if ((e = hipMemsetAsync(ctx->counters, 0, hrt::kNumCounters * sizeof(unsigned long long), ctx->stream)) != hipSuccess)
    return bail(hip_fail(ctx, e, "hipMemset(counters)"));
  // Fresh images read as the cleared state (0,0,0,1) until the first dispatch writes them.
  for (auto& l : ctx->lane)
    if ((e = hrt::launch_clear(l.trace, ctx->f32(), np, ctx->stream)) != hipSuccess) return bail(hip_fail(ctx, e, "clear"));
  if ((e = hrt::launch_clear(ctx->accum, ctx->f32(), np, ctx->stream)) != hipSuccess)
    return bail(hip_fail(ctx, e, "clear"));
  if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(hip_fail(ctx, e, "hipStreamSynchronize"));
  *out_ctx = ctx;
  return HRT_OK;
}

extern "C" void hrt_destroy(hrt_context* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (auto& l : ctx->lane)
    if (l.stream) (void)hipStreamSynchronize(l.stream);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  hrt::comm_release(ctx);
  (void)hipSetDevice(ctx->device);
  hrt::free_scene(ctx, ctx->scene, false);
  for (auto& l : ctx->lane) {
    free_dev(ctx, l.trace);
    free_dev(ctx, l.sched);
    free_dev(ctx, l.tile_cost);
    free_dev(ctx, l.item_buf);
    free_dev(ctx, l.tl_cache);
    if (l.done) (void)hipEventDestroy(l.done);
    if (l.free) (void)hipEventDestroy(l.free);
    if (l.foreign) (void)hipEventDestroy(l.foreign);
    if (l.sky_stream) (void)hipStreamSynchronize(l.sky_stream);
    if (l.sky_fork) (void)hipEventDestroy(l.sky_fork);
    if (l.sky_join) (void)hipEventDestroy(l.sky_join);
    if (l.sky_stream) (void)hipStreamDestroy(l.sky_stream);
    if (l.stream) (void)hipStreamDestroy(l.stream);
  }
  free_dev(ctx, ctx->accum);
  free_dev(ctx, ctx->scratch);
  free_dev(ctx, ctx->counters);
  free_dev(ctx, ctx->tile_cycles);
  free_dev(ctx, ctx->timeline);
  free_dev(ctx, ctx->timeline_count);
  free_dev(ctx, ctx->frame_stack);
  free_dev(ctx, ctx->ring);
  free_dev(ctx, ctx->fold_ring);
  free_dev(ctx, ctx->fold_scratch);
  free_dev(ctx, ctx->query_rays);
  free_dev(ctx, ctx->query_hits);
  free_dev(ctx, ctx->query_stats);
  free_dev(ctx, ctx->occl_bits);
  free_dev(ctx, ctx->occl_stats);
  free_dev(ctx, ctx->rad_out);
  free_dev(ctx, ctx->rad_words);
  free_dev(ctx, ctx->dn_img[0]);
  free_dev(ctx, ctx->dn_img[1]);
  free_dev(ctx, ctx->dn_guide);
  free_dev(ctx, ctx->dn_keys);
  free_dev(ctx, ctx->hist_cnt);
  free_dev(ctx, ctx->hist_cnt_next);
  free_dev(ctx, ctx->hist_accum_next);
  free_dev(ctx, ctx->hist_mom);
  free_dev(ctx, ctx->hist_mom_next);
  free_dev(ctx, ctx->var_stage);
  for (auto& s : ctx->motion_ring) {  // (the streams were drained above: no copy or pass is in flight)
    free_dev(ctx, s.dev);
    if (s.host) (void)hipHostFree(s.host);
    if (s.done) (void)hipEventDestroy(s.done);
  }
  free_dev(ctx, ctx->up_stage);
  free_dev(ctx, ctx->rf_mask);
  free_dev(ctx, ctx->rf_queries);
  free_dev(ctx, ctx->rf_index);
  free_dev(ctx, ctx->rf_rgba);
  free_dev(ctx, ctx->rf_words);
  free_dev(ctx, ctx->rt_bits);
  free_dev(ctx, ctx->rt_counts);
  free_dev(ctx, ctx->rt_sched);
  free_dev(ctx, ctx->rt_items);
  free_dev(ctx, ctx->rt_cost);
  free_dev(ctx, ctx->fh_cam_meta);
  free_dev(ctx, ctx->fh_cam_tris);
  free_dev(ctx, ctx->fh_cam_cull);
  free_dev(ctx, ctx->fh_stats);
  if (ctx->fold_done) (void)hipEventDestroy(ctx->fold_done);
  if (ctx->fold_foreign) (void)hipEventDestroy(ctx->fold_foreign);
  if (ctx->order_ev) (void)hipEventDestroy(ctx->order_ev);
  for (hipEvent_t ev : ctx->present_ev)  // (the streams were drained above: every ticket is complete)
    if (ev) (void)hipEventDestroy(ev);
  for (int i = 0; i < 2; ++i) {
    if (ctx->staging.buf[i]) (void)hipHostFree(ctx->staging.buf[i]);
    if (ctx->staging.ev[i]) (void)hipEventDestroy(ctx->staging.ev[i]);
  }
  for (auto& im : ctx->imports) (void)hipDestroyExternalMemory(im.mem);
  for (auto& ev : ctx->event_pool) {
    (void)hipEventDestroy(ev.start);
    (void)hipEventDestroy(ev.stop);
  }
  for (auto& ev : ctx->pending) {
    (void)hipEventDestroy(ev.start);
    (void)hipEventDestroy(ev.stop);
  }
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

namespace {

// hrt_set_scene's device allocations (the debug build can fail the n-th one: HRT_DEBUG_OPT_FAIL_ALLOC).
struct SceneAlloc {
  hrt_context* ctx;
  int64_t count = 0;
  hipError_t operator()(void** p, size_t bytes) {
    ++count;
    if (ctx->debug_fail_alloc > 0 && count == ctx->debug_fail_alloc) return hipErrorOutOfMemory;
    return hrt::dev_alloc(ctx, p, bytes ? bytes : 16);
  }
};

// Host -> device copy through the context's pinned staging chunks: the CPU fills one chunk while the
// DMA engine drains the other (the reference's upload points, src/raytrace_pipeline.rs:302,337,349,
// 359,371-372, stage through host-visible buffers the same way).
hrt_status stage_upload(hrt_context* ctx, void* dst, const void* src, size_t bytes) {
  auto& s = ctx->staging;
  if (!s.chunk) {  // both chunks and events into locals; published only when all four exist
    void* buf[2] = {};
    hipEvent_t ev[2] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i)
      if ((e = hipHostMalloc(&buf[i], kStagingChunk, hipHostMallocDefault)) == hipSuccess)
        e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
      for (int i = 0; i < 2; ++i) {
        if (buf[i]) (void)hipHostFree(buf[i]);
        if (ev[i]) (void)hipEventDestroy(ev[i]);
      }
      return hip_fail(ctx, e, "hrt_set_scene: pinned staging");
    }
    for (int i = 0; i < 2; ++i) {
      s.buf[i] = buf[i];
      s.ev[i] = ev[i];
      s.used[i] = false;
    }
    s.chunk = kStagingChunk;
  }
  for (size_t off = 0, k = 0; off < bytes; off += s.chunk, ++k) {
    const int i = (int)(k & 1);
    const size_t n = std::min(s.chunk, bytes - off);
    if (s.used[i]) HRT_HIP(ctx, hipEventSynchronize(s.ev[i]));  // the DMA has left this chunk
    std::memcpy(s.buf[i], static_cast<const char*>(src) + off, n);
    HRT_HIP(ctx, hipMemcpyAsync(static_cast<char*>(dst) + off, s.buf[i], n, hipMemcpyHostToDevice, ctx->stream));
    HRT_HIP(ctx, hipEventRecord(s.ev[i], ctx->stream));
    s.used[i] = true;
  }
  return HRT_OK;
}

// Allocate dst (>= 16 B, so empty lists keep a valid pointer) and upload bytes of src into it.
hrt_status alloc_upload(hrt_context* ctx, SceneAlloc& alloc, void** dst, const void* src, size_t bytes,
                        const char* what) {
  if (hipError_t e = alloc(dst, bytes); e != hipSuccess) {
    *dst = nullptr;
    return hip_fail(ctx, e, (std::string("hrt_set_scene: hipMalloc(") + what + ")").c_str());
  }
  return bytes ? stage_upload(ctx, *dst, src, bytes) : HRT_OK;
}

// The band lists' 16-bit image, padded to whole dwords (hrt_kernels.hip band_entry reads dwords).
std::vector<uint16_t> band16(const std::vector<uint32_t>& list) {
  std::vector<uint16_t> v(list.begin(), list.end());
  v.resize((v.size() + 1) & ~(size_t)1, 0);
  return v;
}

// Fills s with a complete device copy of the scene (everything but the kept rays).
hrt_status build_scene(hrt_context* ctx, hrt::SceneBufs& s, const hrt_ray* rays, uint32_t n_rays, bool keep_rays,
                       const hrt_sphere* spheres, uint32_t n_spheres, const hrt_triangle* tris, uint32_t n_tris,
                       const hrt_mesh* meshes, uint32_t n_meshes) {
  SceneAlloc alloc{ctx};
  hrt_status st;
  if (keep_rays)
    s.rays = ctx->scene.rays;
  else if ((st = alloc_upload(ctx, alloc, (void**)&s.rays, rays, (size_t)n_rays * sizeof(float4), "rays")) != HRT_OK)
    return st;
  if ((st = alloc_upload(ctx, alloc, (void**)&s.spheres, spheres, (size_t)n_spheres * 64, "spheres")) != HRT_OK ||
      (st = alloc_upload(ctx, alloc, (void**)&s.tris, tris, (size_t)n_tris * 64, "triangles")) != HRT_OK ||
      (st = alloc_upload(ctx, alloc, (void**)&s.meshes, meshes, (size_t)n_meshes * 80, "meshes")) != HRT_OK)
    return st;
  {  // the hit normal of each triangle, once (resolve_hit reads it instead of normalizing per hit)
    hipError_t e = alloc((void**)&s.tri_nhat, (size_t)(n_tris ? n_tris : 1) * sizeof(float4));
    if (e == hipSuccess) e = hrt::launch_tri_normals(s.tris, s.tri_nhat, n_tris, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "hrt_set_scene: triangle normals");
  }
  uint64_t cap = 0;
  for (uint32_t m = 0; m < n_meshes; ++m) cap += meshes[m].len;
  if (cap > 0xFFFFFFFFull) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_set_scene: too many mesh triangles");
  // bundle-variant buffers, one set per trace lane: per-frame compacted camera-facing records
  for (int l = 0; l < hrt::kLanes; ++l) {
    hipError_t e;
    if ((e = alloc((void**)&s.cam_meta[l], (size_t)(n_meshes ? 2 * n_meshes : 2) * 4)) != hipSuccess ||
        (e = alloc((void**)&s.cam_tris[l], (size_t)(cap ? cap : 1) * 64)) != hipSuccess ||
        (e = alloc((void**)&s.cam_cull[l], (size_t)(cap ? cap : 1) * 80)) != hipSuccess)
      return hip_fail(ctx, e, "hrt_set_scene: hipMalloc(camera lists)");
  }
  s.cam_capacity = (uint32_t)cap;
  // bounce-segment hierarchy (BUNDLE_BVH / BUNDLE_WQ)
  hrt::BvhHost bvh;
  // auto leaf size: 2, 3, then 4 for scenes BUNDLE_WQ takes -- the smallest whose grouped image leaves
  // the LDS stacks kAutoLeafWqStack entries (island: 2; cave: 3, whose leaves of 2 need 104 KB of
  // nodes); 4 above 8192 entries
  uint32_t leaf = ctx->bvh_leaf ? ctx->bvh_leaf : hrt::auto_leaf_size(cap);
  // (the hierarchy alone while the leaf size is chosen, then the band lists once)
  bool built = hrt::build_bvh(tris, n_tris, meshes, n_meshes, leaf, bvh, ctx->bvh_width, hrt::kBandTau, false);
  while (built && ctx->bvh_leaf == 0 && leaf < 4 &&
         !(bvh.wq_ok && hrt::wq_stack_cap(bvh.wq_n_nodes, bvh.wq_width, leaf) >= hrt::kAutoLeafWqStack)) {
    ++leaf;
    built = hrt::build_bvh(tris, n_tris, meshes, n_meshes, leaf, bvh, ctx->bvh_width, hrt::kBandTau, false);
  }
  if (built) hrt::build_bands(bvh);
  const double margin_frac = bvh.margin_frac;
  if (built) {
    auto up = [&](auto*& dst, const auto& v, const char* what) -> hrt_status {
      return alloc_upload(ctx, alloc, (void**)&dst, v.data(), v.size() * sizeof(v[0]), what);
    };
    if ((st = up(s.bvh_nodes, bvh.nodes, "bvh nodes")) != HRT_OK) return st;
    if (bvh.wq_ok && (st = up(s.bvh_wq_nodes, bvh.wq_nodes, "bvh wq nodes")) != HRT_OK) return st;
    // BUNDLE_WQ_L2's image: on the device only for a context that has selected the variant (a later
    // hrt_set_option uploads the host copy, upload_wq_bfs)
    if (bvh.wq_ok && ctx->variant == HRT_KERNEL_BUNDLE_WQ_L2 && !bvh.wq_nodes_bfs.empty() &&
        (st = up(s.bvh_wq_nodes_bfs, bvh.wq_nodes_bfs, "bvh wq nodes (breadth first)")) != HRT_OK)
      return st;
    if (bvh.wq_ok) s.wq_bfs_host = std::move(bvh.wq_nodes_bfs);
    if ((st = up(s.bvh_prims, bvh.prims, "bvh prims")) != HRT_OK ||
        (st = up(s.bvh_irregular, bvh.irregular, "bvh irregular")) != HRT_OK ||
        (st = up(s.bvh_band_off, bvh.band_off, "band offsets")) != HRT_OK ||
        (st = bvh.band_wide() ? up(s.bvh_band, bvh.band_list, "band lists")
                              : up(s.bvh_band, band16(bvh.band_list), "band lists")) != HRT_OK ||
        (st = up(s.bvh_band_nhat, bvh.band_nhat, "band normals")) != HRT_OK ||
        (st = up(s.bvh_entries, bvh.entries, "bvh entries")) != HRT_OK ||
        (st = up(s.bvh_keybase, bvh.key_base, "bvh key bases")) != HRT_OK)
      return st;
    // BUNDLE_WQ's per-cell band records (hrt_kernels.hip band_cell), built on the device from the lists
    // just uploaded: one 32 B record per direction cell (6 x 1,024^2 cells: 201 MB), 16-bit lists only.
    // They only save memory traffic: where they do not fit, the lookups read the offsets and lists (the
    // same bytes, tests/test_gpu_boundary.py::test_failed_set_scene_keeps_the_previous_scene).
    const size_t cells = bvh.band_off.empty() ? 0 : bvh.band_off.size() - 1;
    if (!bvh.band_wide() && cells) {
      hipError_t e = alloc((void**)&s.bvh_band_rec, cells * 32);
      if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();  // (not a sticky error)
        s.bvh_band_rec = nullptr;
      } else if (e == hipSuccess) {
        e = hrt::launch_band_records(s.bvh_band_off, static_cast<const uint32_t*>(s.bvh_band), s.bvh_band_rec,
                                     (uint32_t)cells, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "hrt_set_scene: band records");
      } else {
        return hip_fail(ctx, e, "hrt_set_scene: hipMalloc(band records)");
      }
    }
  }
  s.bvh_info[HRT_SCENE_BVH_NODES] = bvh.n_nodes;
  s.bvh_info[HRT_SCENE_BVH_PRIMS] = bvh.n_prims;
  s.bvh_info[HRT_SCENE_BVH_IRREGULAR] = bvh.n_irregular;
  s.bvh_info[HRT_SCENE_BVH_NEVER] = bvh.n_never;
  s.bvh_info[HRT_SCENE_BVH_BUILT] = built ? 1u : 0u;
  s.bvh_info[HRT_SCENE_BVH_BAND_ENTRIES] = (uint32_t)bvh.band_list.size();
  s.bvh_band_wide = bvh.band_wide() ? 1u : 0u;
  {
    uint32_t longest = 0;
    for (size_t c = 0; c + 1 < bvh.band_off.size(); ++c) longest = std::max(longest, bvh.band_off[c + 1] - bvh.band_off[c]);
    s.bvh_band_bits = 0;
    while (s.bvh_band_bits < 32 && (longest >> s.bvh_band_bits)) ++s.bvh_band_bits;
  }
  s.bvh_info[HRT_SCENE_BVH_SAH_MILLI] = (uint32_t)std::min(1e9, bvh.sah_tri_frac * 1000.0 + 0.5);
  s.bvh_info[HRT_SCENE_BVH_MARGIN_MILLI] = (uint32_t)std::min(1e9, margin_frac * 1000.0 + 0.5);
  s.bvh_abs_coef = bvh.abs_coef;
  s.bvh_band_tau = built ? bvh.band_tau : hrt::kBandTau;
  s.bvh_band_a1 = built ? bvh.band_a1 : 0.0f;
  s.bvh_rel_t = bvh.rel_t;
  s.bvh_dir_res = bvh.dir_res;
  s.bvh_built_leaf = std::max(1u, std::min(leaf, hrt::kBvhMaxLeafCount));  // leaves hold at most this
  s.bvh_wq_n = bvh.wq_ok ? bvh.wq_n_nodes : 0u;
  s.bvh_wq_width = bvh.wq_width;
  s.n_spheres = n_spheres;
  s.n_tris = n_tris;
  s.n_meshes = n_meshes;
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // host arrays are only borrowed
  return HRT_OK;
}

// HRT_OPT_KERNEL_VARIANT = BUNDLE_WQ_L2 on a context whose scene is already set: the breadth-first image's upload.
hrt_status upload_wq_bfs(hrt_context* ctx) {
  hrt::SceneBufs& s = ctx->scene;
  if (!ctx->scene_set || s.bvh_wq_nodes_bfs || s.wq_bfs_host.empty()) return HRT_OK;
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  void* dst = nullptr;
  const size_t bytes = s.wq_bfs_host.size() * sizeof(float);
  if (hipError_t e = hrt::dev_alloc(ctx, &dst, bytes); e != hipSuccess)
    return hip_fail(ctx, e, "hrt_set_option: hipMalloc(bvh wq nodes, breadth first)");
  st = stage_upload(ctx, dst, s.wq_bfs_host.data(), bytes);
  if (st == HRT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess)
    st = fail(ctx, HRT_ERR_HIP, "hrt_set_option: upload of the breadth-first node image");
  if (st != HRT_OK) {
    hrt::dev_free(ctx, dst);
    return st;
  }
  s.bvh_wq_nodes_bfs = static_cast<float4*>(dst);
  return HRT_OK;
}

}  // namespace

extern "C" hrt_status hrt_set_scene(hrt_context* ctx, const hrt_ray* rays, uint32_t n_rays, const hrt_sphere* spheres,
                                    uint32_t n_spheres, const hrt_triangle* tris, uint32_t n_tris,
                                    const hrt_mesh* meshes, uint32_t n_meshes) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const bool keep_rays =
      !rays && n_rays == 0 && ctx->scene.rays && ctx->n_rays == (uint64_t)ctx->width * ctx->height;
  if (!keep_rays && ((uint64_t)n_rays != (uint64_t)ctx->width * ctx->height || !rays))
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT,
                "hrt_set_scene: need width*height rays (or NULL after hrt_generate_rays)");
  if ((n_spheres && !spheres) || (n_tris && !tris) || (n_meshes && !meshes))
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_set_scene: null record array with nonzero count");
  for (uint32_t m = 0; m < n_meshes; ++m) {
    if ((uint64_t)meshes[m].first_index + meshes[m].len > n_tris)
      return fail(ctx, HRT_ERR_INVALID_ARGUMENT,
                  "hrt_set_scene: mesh " + std::to_string(m) + " triangle range exceeds the triangle buffer");
  }
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if ((st = sync_all(ctx)) != HRT_OK) return st;  // no trace in flight reads the buffers replaced below
  // The new scene is built completely beside the old one and swapped in only on success, so a failed
  // call (allocation, upload) leaves the previous scene -- buffers and counts -- intact.
  hrt::SceneBufs s;
  st = build_scene(ctx, s, rays, n_rays, keep_rays, spheres, n_spheres, tris, n_tris, meshes, n_meshes);
  if (st != HRT_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    hrt::free_scene(ctx, s, keep_rays);
    ctx->debug_fail_alloc = 0;
    return st;
  }
  hrt::free_scene(ctx, ctx->scene, keep_rays);
  ctx->scene = s;
  ctx->debug_fail_alloc = 0;
  if (!keep_rays) ctx->n_rays = n_rays;
  for (auto& l : ctx->lane) l.plan_valid = l.cam_ready = l.tl_ready = false;  // costs, camera and tile lists of the old scene
  // the first-hit pass's camera buffers had the old scene's sizes (nothing in flight reads them: sync_all above)
  free_dev(ctx, ctx->fh_cam_meta);
  free_dev(ctx, ctx->fh_cam_tris);
  free_dev(ctx, ctx->fh_cam_cull);
  ctx->fh_cam_meta = nullptr;
  ctx->fh_cam_tris = ctx->fh_cam_cull = nullptr;
  ctx->fh_ready = false;
  ctx->scene_set = true;
  return HRT_OK;
}

namespace {

// The scene and the counts of a push block: everything of check_dispatch but the image size (hrt_radiance).
hrt_status check_counts(hrt_context* ctx, const hrt_push_constants* pc, const char* who) {
  if (!ctx->scene_set) return fail(ctx, HRT_ERR_NO_SCENE, std::string(who) + ": hrt_set_scene has not been called");
  if (pc->num_spheres < 0 || (uint32_t)pc->num_spheres > ctx->scene.n_spheres || pc->num_meshes < 0 ||
      (uint32_t)pc->num_meshes > ctx->scene.n_meshes)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": num_spheres/num_meshes exceed the uploaded scene");
  return HRT_OK;
}

// Validates a dispatch's push block against the context (hrt_trace / hrt_compute_n).
hrt_status check_dispatch(hrt_context* ctx, const hrt_push_constants* pc, const char* who) {
  if (!ctx->scene_set) return fail(ctx, HRT_ERR_NO_SCENE, std::string(who) + ": hrt_set_scene has not been called");
  if (pc->width != ctx->width || pc->height != ctx->height)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": push constant width/height differ from the context");
  return check_counts(ctx, pc, who);
}

// The image a trace writes: the one place that fills TraceParams' (RGBA8 pointer, RGBA32F pointer) pair.
void set_image(hrt::TraceParams& p, const hrt_context* ctx, void* img) {
  p.img8 = ctx->f32() ? nullptr : static_cast<uint32_t*>(img);
  p.img32 = ctx->f32() ? static_cast<float4*>(img) : nullptr;
}

// The kernel argument block of a dispatch of pc into trace lane l's image.
hrt::TraceParams make_params(hrt_context* ctx, const hrt_push_constants* pc, int l) {
  const hrt::SceneBufs& s = ctx->scene;
  const hrt::Lane& lane = ctx->lane[l];
  hrt::TraceParams p{};
  p.rays = s.rays;
  p.spheres = s.spheres;
  p.tris = s.tris;
  p.tri_nhat = s.tri_nhat;
  p.meshes = s.meshes;
  set_image(p, ctx, lane.trace);
  p.counters = ctx->counters_on ? ctx->counters : nullptr;
  p.diag = ctx->diag_on ? ctx->counters + 3 : nullptr;
  p.sky_units = ctx->counters + hrt::kSkyUnitsCounter;
  p.tile_cycles = ctx->diag_on ? ctx->tile_cycles : nullptr;
  p.pc = *pc;
  p.local_rows = ctx->local_rows;
  p.row_tile = ctx->row_tile;
  p.part_index = ctx->part_index;
  p.part_count = ctx->part_count;
  p.n_tris = s.n_tris;
  p.cam_start = s.cam_meta[l];
  p.cam_count = s.cam_meta[l] + s.n_meshes;
  p.cam_list_capacity = s.cam_capacity;
  p.cam_tris = s.cam_tris[l];
  p.cam_cull = s.cam_cull[l];
  p.sec_batch = ctx->sec_batch;
  p.prim_batch = ctx->prim_batch;
  p.sched = lane.sched;
  p.tile_cost = lane.tile_cost;
  p.item_buf = lane.item_buf;
  p.tl_cache = lane.tl_cache;
  p.split_k = ctx->split_k;
  p.split_factor = ctx->split_factor;
  p.split_prio = ctx->split_prio;
  p.coop = ctx->coop;
  p.wq_ncap = ctx->wq_node_cap;  // request; plan_trace sizes the stacks
  p.wq_tcap = ctx->debug_wq_tri_cap;  // (debug) request
  p.grab_always = ctx->debug_grab_runs;  // (debug) frame runs at any size
  p.timeline = ctx->timeline;
  p.timeline_count = ctx->timeline_count;
  p.timeline_cap = ctx->timeline_cap;
  p.plan_valid = lane.plan_valid ? 1u : 0u;
  p.num_cus = ctx->grid_cus ? std::min(ctx->grid_cus, ctx->num_cus) : ctx->num_cus;
  const bool built = s.bvh_info[HRT_SCENE_BVH_BUILT] != 0;
  p.bvh_nodes = built ? s.bvh_nodes : nullptr;
  p.bvh_wq_nodes = built ? s.bvh_wq_nodes : nullptr;
  p.bvh_wq_n_nodes = s.bvh_wq_n;
  p.bvh_wq_width = s.bvh_wq_width;
  p.bvh_wq_nodes_bfs = built ? s.bvh_wq_nodes_bfs : nullptr;
  p.wq_lds_nodes_opt = ctx->wq_lds_nodes;
  p.bvh_prims = s.bvh_prims;
  p.bvh_irregular = s.bvh_irregular;
  p.bvh_band_off = s.bvh_band_off;
  p.bvh_dir_res = s.bvh_dir_res;
  p.bvh_sah_milli = s.bvh_info[HRT_SCENE_BVH_SAH_MILLI];
  p.bvh_band = s.bvh_band;
  p.bvh_band_nhat = s.bvh_band_nhat;
  p.bvh_band_rec = s.bvh_band_rec;
  p.bvh_band_wide = s.bvh_band_wide;
  p.bvh_band_bits = s.bvh_band_bits;
  p.bvh_entries = s.bvh_entries;
  p.bvh_keybase = s.bvh_keybase;
  p.bvh_n_prims = s.bvh_info[HRT_SCENE_BVH_PRIMS];
  p.bvh_n_meshes = s.n_meshes;
  p.bvh_n_nodes = s.bvh_info[HRT_SCENE_BVH_NODES];
  p.bvh_abs_coef = s.bvh_abs_coef;
  p.bvh_rel_t = s.bvh_rel_t;
  p.bvh_band_tau = s.bvh_band_tau;
  p.bvh_band_a1 = s.bvh_band_a1;
  p.bvh_node_r = ctx->wq_node_radius == 2 ||
                 (ctx->wq_node_radius == 0 && s.bvh_info[HRT_SCENE_BVH_MARGIN_MILLI] > hrt::kNodeRadiusMarginMilli);
  p.bvh_n_irregular = s.bvh_info[HRT_SCENE_BVH_IRREGULAR];
  p.bvh_max_leaf = s.bvh_built_leaf;
  p.n_frames = 1;
  p.frame_stride = ctx->npix();
  return p;
}

// One trace launch of p.n_frames frames on `stream` with lane l's planner buffers (timed by a HIP
// event pair counted as that many traces).  masked: a tile-masked launch of a persistent kernel (hrt_refine_tiles):
// no probe, and the lane's costs and plan_valid stay as they are.
hrt_status launch_frames(hrt_context* ctx, hrt::TraceParams& p, hipStream_t stream, int l,
                         const hrt::MaskedPlan* masked = nullptr) {
  if (ctx->diag_on)
    HRT_HIP(ctx, hipMemsetAsync(ctx->tile_cycles, 0, ctx->num_tiles() * 4 * sizeof(unsigned long long), stream));
  if (ctx->timeline) HRT_HIP(ctx, hipMemsetAsync(ctx->timeline_count, 0, sizeof(uint32_t), stream));  // this launch's
  // this launch's plan (hrt_launch_plan.h), shared with its probe: the kernel, and what the host knows of it
  const hrt::LaunchPlan plan = hrt::plan_trace(hrt::plan_scene(p), ctx->variant);
  const hrt::KernelTraits& kernel = hrt::kernel_traits(plan.kernel);
  if (ctx->pending.size() >= kMaxPending) {
    hrt_status st = harvest_one(ctx);
    if (st != HRT_OK) return st;
  }
  hrt::EventPair ev;
  if (!ctx->event_pool.empty()) {
    ev = ctx->event_pool.back();
    ctx->event_pool.pop_back();
  } else {
    HRT_HIP(ctx, hipEventCreate(&ev.start));
    HRT_HIP(ctx, hipEventCreate(&ev.stop));
  }
  ev.frames = p.n_frames > 1 ? p.n_frames : 1u;
  hrt::Lane& lane = ctx->lane[l];
  // camera lists: rebuilt only when the lane's were built for another position (or scene)
  uint32_t key[4];
  std::memcpy(key, p.pc.cam_pos, 12);
  key[3] = p.pc.num_meshes;
  p.cam_lists_ready = lane.cam_ready && std::memcmp(key, lane.cam_key, sizeof key) == 0 ? 1u : 0u;
  lane.cam_ready = false;  // until a launch has rebuilt them
  // the persistent kernels' tile lists (tile_lists): a function of the camera (position, the mat3 the
  // kernels read, jitter), the meshes and the ray centres -- rebuilt when the camera differs from the one
  // they were built for, after hrt_set_scene or hrt_generate_rays, and after a launch of another kernel
  uint32_t tkey[14];
  std::memcpy(tkey, p.pc.cam_pos, 12);
  for (int i = 0, j = 0; i < 11; ++i)
    if (i % 4 != 3) std::memcpy(&tkey[3 + j++], &p.pc.cam_alignment_mat[i], 4);
  std::memcpy(&tkey[12], &p.pc.jitter_size, 4);
  tkey[13] = p.pc.num_meshes;
  p.tl_lists_ready = lane.tl_ready && std::memcmp(tkey, lane.tl_key, sizeof tkey) == 0 ? 1u : 0u;
  lane.tl_ready = false;
  // First trace of a persistent kernel on this lane (no tile costs yet): a 1-sample probe trace into the
  // lane's own image (fully overwritten by the trace that follows on the same stream) measures the
  // tiles' relative costs so that this trace already follows a plan (HRT_OPT_PROBE).
  if (ctx->probe && !lane.plan_valid && ctx->num_tiles() >= 1024 && kernel.persistent && !masked) {
    hrt::TraceParams q = p;
    q.pc.num_samples = 1;
    q.n_frames = 1;
    set_image(q, ctx, lane.trace);
    q.counters = nullptr;
    q.diag = nullptr;
    q.tile_cycles = nullptr;
    q.probe = 1u;
    if (hipError_t pe = hrt::launch_trace(q, plan, stream); pe != hipSuccess) {
      ctx->event_pool.push_back(ev);
      return hip_fail(ctx, pe, "probe trace launch");
    }
    p.plan_valid = 1u;
    if (kernel.camera_lists) p.cam_lists_ready = 1u;  // the probe built them
    p.tl_lists_ready = 1u;                            // (and the tile lists)
  }
  // The sky lane (HRT_OPT_SKY_LANE): BUNDLE_WQ's sky items on trace_sky beside the main kernel, forked from
  // `stream` inside launch_trace and joined back into it there -- so the event pair below spans fork to join
  // and everything that follows on `stream` (folds, reads, the lane's done event) follows the join.  Auto: launches
  // of at least kSkyLaneUnits work units (tile x frame) per resident wave.  Measured on island 1080p:
  // 158 units per wave (the whole frame, 20 frames) 5% faster with the lane; 79 and fewer (10, 5, 2 frames, one
  // frame, a half or an eighth of the rows at 20 or 64 frames) 4-12% slower -- short launches end on the
  // traversal's longest pixel chains, which the capped kernel runs slower, with no sky work left to hide.
  // In the gap: 103 units per wave 3% slower, 127 units 7% faster (island), cave 79 slower, 127 and 158 2% faster.
  // Island 4K at 16 spp and 12 bounces is slower with the lane at 253 and 506 units per wave (2% and 9%), so the
  // rule also asks for the sample count it was measured to win at; everything else keeps the path without the lane.
  // Lane 0 (hrt_compute_n's) warms the side stream with its first BUNDLE_WQ launch, whatever its size.
  constexpr uint64_t kSkyLaneUnits = 128;
  hrt::SkyLane sky{};
  const bool sky_ok = kernel.sky_lane && !ctx->diag_on && !ctx->timeline;
  constexpr int32_t kSkyLaneSamples = 64;
  const bool big = (uint64_t)ctx->num_tiles() * ev.frames >= kSkyLaneUnits * p.num_cus * 16u &&
                   p.pc.num_samples >= kSkyLaneSamples;
  const bool run_sky = sky_ok && (ctx->sky_lane > 0 || (ctx->sky_lane < 0 && big));
  const bool want_sky = run_sky || (sky_ok && ctx->sky_lane < 0 && l == 0 && !lane.sky_stream);
  if (want_sky) {
    hipError_t se = hipSuccess;
    // The side stream has the lowest stream priority: the runtime keeps a pool of hardware queues per priority,
    // so trace_sky never shares a queue with a trace lane's or the context's stream, whatever other streams the
    // process has made (streams of one priority share up to four queues in turn: with the main kernel's stream
    // on the same queue trace_sky would start after it had ended, find the plan empty, and leave the capped
    // main kernel to run alone -- seen in a process's second context, with hrt_debug_sky_units at 0).
    if (!lane.sky_stream) {
      int least = 0, greatest = 0;
      se = hipDeviceGetStreamPriorityRange(&least, &greatest);
      if (se == hipSuccess) se = hipStreamCreateWithPriority(&lane.sky_stream, hipStreamNonBlocking, least);
    }
    if (se == hipSuccess && !lane.sky_fork) se = hipEventCreateWithFlags(&lane.sky_fork, hipEventDisableTiming);
    if (se == hipSuccess && !lane.sky_join) se = hipEventCreateWithFlags(&lane.sky_join, hipEventDisableTiming);
    if (se != hipSuccess) {
      ctx->event_pool.push_back(ev);
      return hip_fail(ctx, se, "sky lane stream / events");
    }
    sky = hrt::SkyLane{lane.sky_stream, lane.sky_fork, lane.sky_join, run_sky};
  }
  HRT_HIP(ctx, hipEventRecord(ev.start, stream));
  ctx->last_kernel = plan.kernel;
  ctx->last_block = (int)plan.block;
  hipError_t e = hrt::launch_trace(p, plan, stream, want_sky ? &sky : nullptr, masked);
  if (e == hipSuccess) ctx->last_frames = ev.frames;
  // the persistent kernels recorded this trace's tile costs: the lane's next trace can follow a plan
  if (!masked) lane.plan_valid = e == hipSuccess && kernel.persistent;  // (a masked launch recorded into its own image)
  // (only a kernel that built the lists leaves them valid: a LITERAL / BRUTE trace from this position
  // followed by a bundle kernel must rebuild them)
  if (e == hipSuccess && kernel.camera_lists) {
    lane.cam_ready = true;
    std::memcpy(lane.cam_key, key, sizeof key);
  }
  if (e == hipSuccess && kernel.persistent) {
    lane.tl_ready = true;
    std::memcpy(lane.tl_key, tkey, sizeof tkey);
  }
  if (e != hipSuccess) {
    ctx->event_pool.push_back(ev);
    return hip_fail(ctx, e, "trace kernel launch");
  }
  HRT_HIP(ctx, hipEventRecord(ev.stop, stream));
  ctx->pending.push_back(ev);
  ctx->traces += ev.frames;
  return HRT_OK;
}

// The deferred combiner's ring of frame images: up to 16 frames within 512 MiB; none (immediate
// combines) when fewer than 4 frames fit.  Allocated once, by the first trace that needs it.
constexpr size_t kRingBytes = (size_t)512 << 20;
hrt_status ensure_ring(hrt_context* ctx) {
  if (ctx->ring || ctx->ring_n == 0xFFFFFFFFu) return HRT_OK;
  const size_t fb = ctx->npix() * ctx->px_bytes();
  const size_t n = std::min<size_t>(16, kRingBytes / std::max<size_t>(fb, 1));
  if (n < 4) {
    ctx->ring_n = 0xFFFFFFFFu;  // (never: frames this large combine immediately)
    return HRT_OK;
  }
  HRT_HIP(ctx, hrt::dev_alloc(ctx, &ctx->ring, n * fb));
  ctx->ring_n = (uint32_t)n;
  ctx->ring_next = 0;
  return HRT_OK;
}

// The lane the next trace runs on (rotating over HRT_OPT_OVERLAP lanes, after the lane's last reader).
hrt_status begin_lane(hrt_context* ctx, int* out) {
  // (diagnostics and the timeline record into one buffer per context: one lane, so no two launches
  // interleave their records or reset each other's count -- ADVICE r05)
  const int n = ctx->diag_on || ctx->timeline ? 1 : (int)std::max(1u, ctx->overlap);
  const int l = ctx->lane_used ? (ctx->cur_lane + 1) % n : 0;
  hrt::Lane& lane = ctx->lane[l];
  if (lane.free_set) HRT_HIP(ctx, hipStreamWaitEvent(lane.stream, lane.free, 0));
  // ... and after a reader on another context's stream (hrt_accumulate_history_from)
  if (lane.foreign_set) HRT_HIP(ctx, hipStreamWaitEvent(lane.stream, lane.foreign, 0));
  *out = l;
  return HRT_OK;
}

hrt_status end_lane(hrt_context* ctx, int l) {
  HRT_HIP(ctx, hipEventRecord(ctx->lane[l].done, ctx->lane[l].stream));
  ctx->lane[l].done_set = true;
  ctx->cur_lane = l;
  ctx->lane_used = true;
  return HRT_OK;
}

}  // namespace

extern "C" hrt_status hrt_trace(hrt_context* ctx, const hrt_push_constants* pc) {
  if (!ctx || !pc) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if (!pc->init && (st = check_dispatch(ctx, pc, "hrt_trace")) != HRT_OK) return st;
  // The frame's image: the next ring slot when combines are deferred (the ring is allocated by the
  // first such trace; a slot still waiting for its fold forces the fold first), else the lane's own.
  int slot = -1;
  if (!pc->init && ctx->defer) {
    if ((st = ensure_ring(ctx)) != HRT_OK) return st;
    if (ctx->ring) {
      slot = (int)ctx->ring_next;
      // (the flush clears ctx->pend: decide first, flush outside the loop)
      const bool busy = std::any_of(ctx->pend.begin(), ctx->pend.end(),
                                    [&](const auto& pd) { return pd.slot == (uint32_t)slot; });
      if (busy && (st = hrt::flush_combines(ctx)) != HRT_OK) return st;
    }
  }
  int l = 0;
  if ((st = begin_lane(ctx, &l)) != HRT_OK) return st;
  hrt::Lane& lane = ctx->lane[l];
  if (pc->init) {  // RayTracePipeline::init, src/raytrace_pipeline.rs:190-213
    HRT_HIP(ctx, hrt::launch_clear(lane.trace, ctx->f32(), ctx->npix(), lane.stream));
  } else {
    hrt::TraceParams p = make_params(ctx, pc, l);
    if (slot >= 0) {  // after the fold that last read the slot
      if (ctx->fold_set) HRT_HIP(ctx, hipStreamWaitEvent(lane.stream, ctx->fold_done, 0));
      if (ctx->fold_foreign_set) HRT_HIP(ctx, hipStreamWaitEvent(lane.stream, ctx->fold_foreign, 0));
      set_image(p, ctx, static_cast<char*>(ctx->ring) + (size_t)slot * ctx->npix() * ctx->px_bytes());
    }
    // Throughput mode: when another lane's trace is still running, this one shares the chip with it
    // (a persistent grid over 1 / HRT_OPT_BUSY_SPLIT of the CUs), so two frames' long sample chains run
    // side by side instead of the next frame waiting for every CU; an idle GPU gets the whole grid.
    if (ctx->busy_split > 1) {
      bool busy = false;
      for (int o = 0; o < hrt::kLanes; ++o)
        if (o != l && ctx->lane[o].done_set && hipEventQuery(ctx->lane[o].done) == hipErrorNotReady) busy = true;
      if (busy) p.num_cus = std::max(1u, p.num_cus / ctx->busy_split);
    }
    if ((st = launch_frames(ctx, p, lane.stream, l)) != HRT_OK) return st;
  }
  ctx->cur_slot = slot;
  if (slot >= 0) ctx->ring_next = (uint32_t)(slot + 1) % ctx->ring_n;
  return end_lane(ctx, l);
}

// ---- ray queries ---------------------------------------------------------------------
namespace {

constexpr uint32_t kQueryChunk = 1u << 16;   // rays per staged chunk (2 MiB of rays, 2 MiB of hits)
constexpr uint32_t kQueryLaunch = 1u << 24;  // rays per launch when nothing is staged

// Whether a kernel of this context reads / writes p directly: memory of its device or managed memory.
// Anything else (pageable or registered host memory, another device's) goes through the staging buffers.
bool query_direct(hrt_context* ctx, const void* p) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // (an unknown pointer is not a sticky error)
    return false;
  }
  return (at.type == hipMemoryTypeDevice && at.device == ctx->device) || at.type == hipMemoryTypeManaged;
}

// A query writes no image, counter or planner buffer of the context.
void query_only(hrt::TraceParams& p) {
  p.img8 = nullptr;
  p.img32 = nullptr;
  p.counters = nullptr;
  p.diag = nullptr;
  p.tile_cycles = nullptr;
  p.sky_units = nullptr;
  p.timeline = nullptr;
  p.timeline_count = nullptr;
}

// A staging or statistics buffer of the queries, allocated at its first use (the context's allocator).
hrt_status ensure_staging(hrt_context* ctx, void** buf, size_t bytes, const char* who) {
  if (*buf) return HRT_OK;
  if (hrt::dev_alloc(ctx, buf, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, HRT_ERR_OUT_OF_MEMORY, std::string(who) + ": staging allocation failed");
  }
  return HRT_OK;
}

// n rays (rays, or, when rays is null, the primary rays k = 0 .. n - 1 of rect) -> hits, blocking.  Every
// argument has been checked; p.pc holds the counts (and the camera).
hrt_status run_query(hrt_context* ctx, hrt::TraceParams p, const hrt_ray_query* rays, uint32_t n, const uint32_t rect[3],
                     uint32_t method, hrt_hit* hits, hrt_query_stats* stats, const char* who) {
  const bool primary = rays == nullptr;
  query_only(p);
  const hrt::QueryPlan plan = hrt::plan_query(hrt::plan_scene(p), (int)method);
  const bool rays_direct = primary || query_direct(ctx, rays), hits_direct = query_direct(ctx, hits);
  if ((!primary && rays_direct && (uintptr_t)rays % 16 != 0) || (hits_direct && (uintptr_t)hits % 16 != 0))
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": device rays / hits must be 16-byte aligned");
  auto ensure = [&](void** buf, size_t bytes) { return ensure_staging(ctx, buf, bytes, who); };
  hrt_status st;
  if (!rays_direct && (st = ensure(&ctx->query_rays, (size_t)kQueryChunk * sizeof(hrt_ray_query))) != HRT_OK) return st;
  if (!hits_direct && (st = ensure(&ctx->query_hits, (size_t)kQueryChunk * sizeof(hrt_hit))) != HRT_OK) return st;
  if (stats) {
    if ((st = ensure(reinterpret_cast<void**>(&ctx->query_stats), 2 * sizeof(unsigned long long))) != HRT_OK) return st;
    HRT_HIP(ctx, hipMemsetAsync(ctx->query_stats, 0, 2 * sizeof(unsigned long long), ctx->stream));
  }
  const uint32_t chunk = (rays_direct && hits_direct) ? kQueryLaunch : kQueryChunk;
  for (uint32_t at = 0; at < n; at += std::min(chunk, n - at)) {
    const uint32_t m = std::min(chunk, n - at);
    hrt::QueryArgs q{};
    if (!primary) {
      if (rays_direct) {
        q.rays = reinterpret_cast<const float4*>(rays + at);
      } else {
        HRT_HIP(ctx, hipMemcpyAsync(ctx->query_rays, rays + at, (size_t)m * sizeof(hrt_ray_query), hipMemcpyDefault,
                                    ctx->stream));
        q.rays = static_cast<const float4*>(ctx->query_rays);
      }
    }
    q.hits = hits_direct ? reinterpret_cast<float4*>(hits + at) : static_cast<float4*>(ctx->query_hits);
    q.stats = stats ? ctx->query_stats : nullptr;
    q.n = m;
    q.first = at;
    q.x0 = rect[0];
    q.y0 = rect[1];
    q.w = rect[2];
    HRT_HIP(ctx, hrt::launch_query(p, q, plan, primary, ctx->stream));
    if (!hits_direct)
      HRT_HIP(ctx, hipMemcpyAsync(hits + at, ctx->query_hits, (size_t)m * sizeof(hrt_hit), hipMemcpyDefault, ctx->stream));
  }
  unsigned long long counts[2] = {0, 0};
  if (stats) HRT_HIP(ctx, hipMemcpyAsync(counts, ctx->query_stats, sizeof(counts), hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) *stats = hrt_query_stats{(uint32_t)plan.method, 0u, counts[0], counts[1]};
  return HRT_OK;
}

bool known_query_method(uint32_t method) {
  // the four methods of hrt_query_method
  return method <= HRT_QUERY_PAIRS;
}

}  // namespace

extern "C" hrt_status hrt_intersect(hrt_context* ctx, const hrt_ray_query* rays, uint32_t n, uint32_t method,
                                    hrt_hit* hits, hrt_query_stats* stats) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  if (!known_query_method(method)) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_intersect: unknown method");
  if (!ctx->scene_set) return fail(ctx, HRT_ERR_NO_SCENE, "hrt_intersect: hrt_set_scene has not been called");
  if (n > 0 && (!rays || !hits)) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_intersect: null rays or hits");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  hrt_push_constants pc{};
  pc.width = ctx->width;
  pc.height = ctx->height;
  pc.num_spheres = (int32_t)ctx->scene.n_spheres;
  pc.num_meshes = (int32_t)ctx->scene.n_meshes;
  const hrt::TraceParams p = make_params(ctx, &pc, 0);
  if (n == 0) {
    if (stats) *stats = hrt_query_stats{(uint32_t)hrt::plan_query(hrt::plan_scene(p), (int)method).method, 0u, 0u, 0u};
    return HRT_OK;
  }
  const uint32_t rect[3] = {0, 0, 1};
  return run_query(ctx, p, rays, n, rect, method, hits, stats, "hrt_intersect");
}

extern "C" hrt_status hrt_intersect_primary(hrt_context* ctx, const hrt_push_constants* pc, uint32_t x0, uint32_t y0,
                                            uint32_t w, uint32_t h, uint32_t method, hrt_hit* hits,
                                            hrt_query_stats* stats) {
  if (!ctx || !pc) return HRT_ERR_INVALID_ARGUMENT;
  if (!known_query_method(method)) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_intersect_primary: unknown method");
  hrt_status st = check_dispatch(ctx, pc, "hrt_intersect_primary");
  if (st != HRT_OK) return st;
  if (x0 > ctx->width || w > ctx->width - x0 || y0 > ctx->height || h > ctx->height - y0)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_intersect_primary: the rectangle lies outside the image");
  const uint64_t n = (uint64_t)w * h;
  if (n > 0xFFFFFFFFull) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_intersect_primary: more than 2^32 - 1 pixels");
  if (n > 0 && !hits) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_intersect_primary: null hits");
  if ((st = bind(ctx)) != HRT_OK) return st;
  const hrt::TraceParams p = make_params(ctx, pc, 0);
  if (n == 0) {
    if (stats) *stats = hrt_query_stats{(uint32_t)hrt::plan_query(hrt::plan_scene(p), (int)method).method, 0u, 0u, 0u};
    return HRT_OK;
  }
  const uint32_t rect[3] = {x0, y0, w};
  return run_query(ctx, p, nullptr, (uint32_t)n, rect, method, hits, stats, "hrt_intersect_primary");
}

// ---- the first-hit pass ------------------------------------------------------------
// The whole image's first hits enqueued on ctx->stream with no host wait.  TILES owns a fourth set of camera
// buffers, so the pass never touches a lane's lists or their keys; QUERY is hrt_intersect_primary's AUTO kernel
// without the synchronise.
namespace {
// AUTO: TILES, which beat QUERY on island and on cave at 1080p from a fresh camera with the five-run ranges
// apart -- island 0.15 ms against 0.23, cave 0.11 against 0.53 (profiles/first_hits_rate.jsonl)
constexpr uint32_t kFirstHitsAuto = HRT_FIRST_HITS_TILES;
}  // namespace

extern "C" hrt_status hrt_first_hits(hrt_context* ctx, const hrt_push_constants* pc, uint32_t method, uint32_t flags,
                                     hrt_hit* hits) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string("hrt_first_hits: ") + what); };
  if (!pc) return bad("null push block");
  if (!hits) return bad("null hits");
  if (method > HRT_FIRST_HITS_QUERY) return bad("unknown method");
  if (flags & ~HRT_FIRST_HITS_COUNT) return bad("flag bits other than HRT_FIRST_HITS_COUNT");
  if (ctx->comm || ctx->part_count > 1)
    return bad("a context of a row-tile partition or joined to a communicator has no first-hit pass (its consumers, "
               "hrt_reproject and hrt_denoise, refuse such a context)");
  hrt_status st = check_dispatch(ctx, pc, "hrt_first_hits");
  if (st != HRT_OK) return st;
  if ((st = bind(ctx)) != HRT_OK) return st;
  if ((uintptr_t)hits % 16 != 0) return bad("hits must be 16-byte aligned");
  if (!query_direct(ctx, hits) || !query_direct(ctx, hits + (ctx->npix() - 1)))
    return bad("hits must be width x height records in memory of the context's device");
  const bool count = (flags & HRT_FIRST_HITS_COUNT) != 0;
  const uint32_t ran = method == HRT_FIRST_HITS_AUTO ? kFirstHitsAuto : method;
  const char* who = "hrt_first_hits";
  if (count) {
    void* s = ctx->fh_stats;
    if ((st = ensure_staging(ctx, &s, hrt::kFirstHitsStatWords * sizeof(unsigned long long), who)) != HRT_OK) return st;
    ctx->fh_stats = static_cast<unsigned long long*>(s);
  }
  hrt::TraceParams p = make_params(ctx, pc, 0);
  query_only(p);
  const uint32_t n = ctx->width * ctx->height;  // (= the scene's ray count, a uint32)
  if (ran == HRT_FIRST_HITS_TILES) {
    const hrt::SceneBufs& sb = ctx->scene;
    void *meta = ctx->fh_cam_meta, *tris = ctx->fh_cam_tris, *cull = ctx->fh_cam_cull;
    // (the lanes' sizes: build_scene)
    if ((st = ensure_staging(ctx, &meta, (size_t)(sb.n_meshes ? 2 * sb.n_meshes : 2) * 4, who)) != HRT_OK) return st;
    ctx->fh_cam_meta = static_cast<uint32_t*>(meta);
    if ((st = ensure_staging(ctx, &tris, (size_t)(sb.cam_capacity ? sb.cam_capacity : 1) * 64, who)) != HRT_OK) return st;
    ctx->fh_cam_tris = static_cast<float4*>(tris);
    if ((st = ensure_staging(ctx, &cull, (size_t)(sb.cam_capacity ? sb.cam_capacity : 1) * 80, who)) != HRT_OK) return st;
    ctx->fh_cam_cull = static_cast<float4*>(cull);
    p.cam_start = ctx->fh_cam_meta;
    p.cam_count = ctx->fh_cam_meta + sb.n_meshes;
    p.cam_tris = ctx->fh_cam_tris;
    p.cam_cull = ctx->fh_cam_cull;
    p.tl_cache = nullptr;
    p.pc.jitter_size = 0.0f;  // the lists' reach: the un-jittered centre is each pixel's whole box
    uint32_t key[4];
    std::memcpy(key, pc->cam_pos, 12);
    key[3] = (uint32_t)pc->num_meshes;
    const bool ready = ctx->fh_ready && std::memcmp(key, ctx->fh_key, sizeof key) == 0;
    if (count) HRT_HIP(ctx, hipMemsetAsync(ctx->fh_stats, 0, hrt::kFirstHitsStatWords * sizeof(unsigned long long), ctx->stream));
    ctx->fh_ready = false;  // until a launch has rebuilt them
    const hrt::FirstHitsArgs a{reinterpret_cast<float4*>(hits), count ? ctx->fh_stats : nullptr};
    HRT_HIP(ctx, hrt::launch_first_hits_tiles(p, a, ready, ctx->stream));
    ctx->fh_ready = true;
    std::memcpy(ctx->fh_key, key, sizeof key);
  } else {
    const hrt::QueryPlan plan = hrt::plan_query(hrt::plan_scene(p), HRT_QUERY_AUTO);
    if (count) HRT_HIP(ctx, hipMemsetAsync(ctx->fh_stats, 0, hrt::kFirstHitsStatWords * sizeof(unsigned long long), ctx->stream));
    for (uint32_t at = 0; at < n; at += std::min(kQueryLaunch, n - at)) {
      hrt::QueryArgs q{};
      q.hits = reinterpret_cast<float4*>(hits + at);
      q.stats = count ? ctx->fh_stats : nullptr;  // words 0 and 1 are hrt_query_stats' two
      q.n = std::min(kQueryLaunch, n - at);
      q.first = at;
      q.w = ctx->width;
      HRT_HIP(ctx, hrt::launch_query(p, q, plan, true, ctx->stream));
    }
  }
  if (count) {
    ctx->fh_counted_method = ran;
    ctx->fh_counted_tiles = ran == HRT_FIRST_HITS_TILES ? (uint32_t)(((ctx->width + 7) / 8) * ((ctx->height + 7) / 8)) : 0u;
  }
  return HRT_OK;
}

extern "C" hrt_status hrt_get_first_hits_stats(hrt_context* ctx, hrt_first_hits_stats* out) {
  if (!ctx || !out) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  unsigned long long w[hrt::kFirstHitsStatWords] = {};
  if (ctx->fh_counted_method != 0)
    HRT_HIP(ctx, hipMemcpyAsync(w, ctx->fh_stats, sizeof w, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *out = hrt_first_hits_stats{ctx->fh_counted_method, 0u, ctx->fh_counted_tiles, (uint32_t)w[2], (uint32_t)w[3],
                              (uint32_t)w[4], w[0], w[1], w[5]};
  return HRT_OK;
}

// Any hit, one bit per ray.  A chunk of staged rays or bits is kQueryChunk rays -- a multiple
// of 64, so every launch but the last fills whole words (2,048 per chunk) and a wave's two words never
// straddle two launches.
extern "C" hrt_status hrt_occluded(hrt_context* ctx, const hrt_ray_query* rays, uint32_t n, uint32_t method,
                                   uint32_t* bits, hrt_occlusion_stats* stats) {
  static_assert(kQueryChunk % 64u == 0 && kQueryLaunch % 64u == 0, "a launch's first ray is a multiple of 64");
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  if (!known_query_method(method)) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_occluded: unknown method");
  if (!ctx->scene_set) return fail(ctx, HRT_ERR_NO_SCENE, "hrt_occluded: hrt_set_scene has not been called");
  if (n > 0 && (!rays || !bits)) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_occluded: null rays or bits");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  hrt_push_constants pc{};
  pc.width = ctx->width;
  pc.height = ctx->height;
  pc.num_spheres = (int32_t)ctx->scene.n_spheres;
  pc.num_meshes = (int32_t)ctx->scene.n_meshes;
  hrt::TraceParams p = make_params(ctx, &pc, 0);
  const hrt::QueryPlan plan = hrt::plan_query(hrt::plan_scene(p), (int)method);
  if (n == 0) {
    if (stats) *stats = hrt_occlusion_stats{(uint32_t)plan.method, 0u, 0u, 0u, 0u};
    return HRT_OK;
  }
  query_only(p);
  const bool rays_direct = query_direct(ctx, rays), bits_direct = query_direct(ctx, bits);
  if (rays_direct && (uintptr_t)rays % 16 != 0)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_occluded: device rays must be 16-byte aligned");
  if (bits_direct && (uintptr_t)bits % 4 != 0)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_occluded: device bits must be 4-byte aligned");
  auto ensure = [&](void** buf, size_t bytes) { return ensure_staging(ctx, buf, bytes, "hrt_occluded"); };
  if (!rays_direct && (st = ensure(&ctx->query_rays, (size_t)kQueryChunk * sizeof(hrt_ray_query))) != HRT_OK) return st;
  if (!bits_direct && (st = ensure(&ctx->occl_bits, (size_t)(kQueryChunk / 32u) * sizeof(uint32_t))) != HRT_OK) return st;
  if (stats) {
    if ((st = ensure(reinterpret_cast<void**>(&ctx->occl_stats), 3 * sizeof(unsigned long long))) != HRT_OK) return st;
    HRT_HIP(ctx, hipMemsetAsync(ctx->occl_stats, 0, 3 * sizeof(unsigned long long), ctx->stream));
  }
  const uint32_t chunk = (rays_direct && bits_direct) ? kQueryLaunch : kQueryChunk;
  for (uint32_t at = 0; at < n; at += std::min(chunk, n - at)) {
    const uint32_t m = std::min(chunk, n - at), words = (m + 31u) / 32u;
    hrt::QueryArgs q{};
    if (rays_direct) {
      q.rays = reinterpret_cast<const float4*>(rays + at);
    } else {
      HRT_HIP(ctx, hipMemcpyAsync(ctx->query_rays, rays + at, (size_t)m * sizeof(hrt_ray_query), hipMemcpyDefault,
                                  ctx->stream));
      q.rays = static_cast<const float4*>(ctx->query_rays);
    }
    q.stats = stats ? ctx->occl_stats : nullptr;
    q.n = m;
    uint32_t* out = bits_direct ? bits + at / 32u : static_cast<uint32_t*>(ctx->occl_bits);
    HRT_HIP(ctx, hrt::launch_occluded(p, q, out, plan, ctx->stream));
    if (!bits_direct)
      HRT_HIP(ctx, hipMemcpyAsync(bits + at / 32u, ctx->occl_bits, (size_t)words * sizeof(uint32_t), hipMemcpyDefault,
                                  ctx->stream));
  }
  unsigned long long counts[3] = {0, 0, 0};
  if (stats) HRT_HIP(ctx, hipMemcpyAsync(counts, ctx->occl_stats, sizeof(counts), hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) *stats = hrt_occlusion_stats{(uint32_t)plan.method, 0u, counts[0], counts[1], counts[2]};
  return HRT_OK;
}

// The path tracer for caller-chosen samples.  Staged records use the ray queries'
// buffer (both records are 32 bytes); ctx->rad_words holds the call's three counts and, after them, the PAIRS
// kernel's query counter, which launch_radiance zeroes before every launch.
extern "C" hrt_status hrt_radiance(hrt_context* ctx, const hrt_push_constants* pc, const hrt_radiance_query* queries,
                                   uint32_t n, uint32_t method, float* rgba, hrt_radiance_stats* stats) {
  static_assert(sizeof(hrt_radiance_query) == sizeof(hrt_ray_query), "one staging buffer for both");
  if (!ctx || !pc) return HRT_ERR_INVALID_ARGUMENT;
  if (!known_query_method(method)) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_radiance: unknown method");
  if (pc->init) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_radiance: pc->init must be 0");
  hrt_status st = check_counts(ctx, pc, "hrt_radiance");
  if (st != HRT_OK) return st;
  if (n > 0 && (!queries || !rgba)) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_radiance: null queries or rgba");
  if ((st = bind(ctx)) != HRT_OK) return st;
  hrt::TraceParams p = make_params(ctx, pc, 0);
  // AUTO: the pair traversal when it fits -- every segment after a query's first is a bounce ray (§26)
  const hrt::QueryPlan plan =
      hrt::plan_query(hrt::plan_scene(p), method == HRT_QUERY_AUTO ? (int)HRT_QUERY_PAIRS : (int)method);
  if (n == 0) {
    if (stats) *stats = hrt_radiance_stats{(uint32_t)plan.method, 0u, 0u, 0u, 0u};
    return HRT_OK;
  }
  query_only(p);
  const bool q_direct = query_direct(ctx, queries), out_direct = query_direct(ctx, rgba);
  if ((q_direct && (uintptr_t)queries % 16 != 0) || (out_direct && (uintptr_t)rgba % 16 != 0))
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_radiance: device queries / rgba must be 16-byte aligned");
  auto ensure = [&](void** buf, size_t bytes) { return ensure_staging(ctx, buf, bytes, "hrt_radiance"); };
  if (!q_direct && (st = ensure(&ctx->query_rays, (size_t)kQueryChunk * sizeof(hrt_radiance_query))) != HRT_OK) return st;
  if (!out_direct && (st = ensure(&ctx->rad_out, (size_t)kQueryChunk * 4 * sizeof(float))) != HRT_OK) return st;
  if ((st = ensure(reinterpret_cast<void**>(&ctx->rad_words), 4 * sizeof(unsigned long long))) != HRT_OK) return st;
  if (stats) HRT_HIP(ctx, hipMemsetAsync(ctx->rad_words, 0, 3 * sizeof(unsigned long long), ctx->stream));
  const uint32_t chunk = (q_direct && out_direct) ? kQueryLaunch : kQueryChunk;
  for (uint32_t at = 0; at < n; at += std::min(chunk, n - at)) {
    const uint32_t m = std::min(chunk, n - at);
    hrt::RadianceArgs q{};
    if (q_direct) {
      q.queries = reinterpret_cast<const float4*>(queries + at);
    } else {
      HRT_HIP(ctx, hipMemcpyAsync(ctx->query_rays, queries + at, (size_t)m * sizeof(hrt_radiance_query),
                                  hipMemcpyDefault, ctx->stream));
      q.queries = static_cast<const float4*>(ctx->query_rays);
    }
    q.out = out_direct ? reinterpret_cast<float4*>(rgba + 4 * (size_t)at) : static_cast<float4*>(ctx->rad_out);
    q.stats = stats ? ctx->rad_words : nullptr;
    q.next = reinterpret_cast<uint32_t*>(ctx->rad_words + 3);
    q.n = m;
    HRT_HIP(ctx, hrt::launch_radiance(p, q, plan, ctx->stream));
    if (!out_direct)
      HRT_HIP(ctx, hipMemcpyAsync(rgba + 4 * (size_t)at, ctx->rad_out, (size_t)m * 4 * sizeof(float), hipMemcpyDefault,
                                  ctx->stream));
  }
  unsigned long long counts[3] = {0, 0, 0};
  if (stats) HRT_HIP(ctx, hipMemcpyAsync(counts, ctx->rad_words, sizeof(counts), hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) *stats = hrt_radiance_stats{(uint32_t)plan.method, 0u, counts[0], counts[1], counts[2]};
  return HRT_OK;
}

// The frame stack's allocation (the debug build can make it fail above HRT_DEBUG_OPT_STACK_LIMIT bytes).
static hipError_t stack_alloc(hrt_context* ctx, void** p, size_t bytes) {
#ifdef HRT_DEBUG_OPTIONS
  if (ctx->debug_stack_limit > 0 && bytes > (size_t)ctx->debug_stack_limit) return hipErrorOutOfMemory;
#endif
  return hrt::dev_alloc(ctx, p, bytes);
}

// hrt_compute_n / hrt_compute_until: grows the frame stack towards a whole launch of cap frames for a call of
// n frames (the policy is described in hrt_compute_n).  Never an error for a stack that does not fit.
static hrt_status grow_frame_stack(hrt_context* ctx, uint32_t cap, uint32_t n, size_t np, size_t px_bytes) {
  if (ctx->frame_stack_frames < cap) {
    const uint32_t need = std::min(cap, n);
    void* fresh = nullptr;
    uint32_t fresh_frames = 0;
    auto try_alloc = [&](uint32_t frames) {
      if (stack_alloc(ctx, &fresh, (size_t)frames * np * px_bytes) == hipSuccess) {
        fresh_frames = frames;
        return true;
      }
      (void)hipGetLastError();  // (a failed allocation is not a sticky error)
      fresh = nullptr;
      return false;
    };
    if (ctx->frame_stack_failed != cap && !try_alloc(cap)) ctx->frame_stack_failed = cap;
    if (!fresh && ctx->frame_stack_frames < need) (void)try_alloc(need);
    if (fresh) {
      HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
      free_dev(ctx, ctx->frame_stack);
      ctx->frame_stack = fresh;
      ctx->frame_stack_frames = fresh_frames;
    }
  }
  return HRT_OK;
}

// ---- the batched loops (hrt_compute_n, hrt_compute_until): lane 0's buffers on the context stream ----
namespace {

// A call's parameter block and its frames per launch (1: one launch per frame).
struct Batch {
  hrt::TraceParams p;
  uint32_t lcap;
};

// The whole loop runs on the context stream with lane 0's buffers, after every lane's last trace
// and every deferred combine (frames fold in call order).  Frames per launch: up to
// HRT_OPT_FRAMES_PER_LAUNCH and `bound`, and at most 1 GiB of frame images.
// The stack is sized for a whole launch of cap frames at once (a stack grown from a short first call --
// bench.py's 5 warm-up frames -- was re-allocated by the next longer call, a device synchronisation and
// ~0.3 ms of hipFree / hipMalloc inside that call).  Where that does not fit (several contexts on one
// device, little free memory) the call's own min(cap, n) frames are allocated instead; where even those
// do not fit, the call runs with the stack it has (more, shorter launches) or one launch per frame.
// Never an error: the frames are the same bytes whatever the launches hold.
hrt_status begin_batch(hrt_context* ctx, const hrt_push_constants* pc, uint32_t n, uint32_t bound, Batch* b) {
  hrt_status st;
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;
  if ((st = hrt::join_lanes(ctx)) != HRT_OK) return st;
  // lane 0's image is written on this stream: after another context's fold that still reads it
  if (ctx->lane[0].foreign_set) HRT_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->lane[0].foreign, 0));
  b->p = make_params(ctx, pc, 0);
  const size_t np = ctx->npix(), px_bytes = ctx->px_bytes();
  const uint32_t cap = (uint32_t)std::max<size_t>(
      1, std::min<size_t>(std::min(ctx->frames_per_launch, bound), ((size_t)1 << 30) / std::max<size_t>(np * px_bytes, 1)));
  const hrt::LaunchPlan plan = hrt::plan_trace(hrt::plan_scene(b->p), ctx->variant);
  const bool batch = hrt::kernel_traits(plan.kernel).persistent && cap > 1 && n > 1;
  if (batch && (st = grow_frame_stack(ctx, cap, n, np, px_bytes)) != HRT_OK) return st;
  b->lcap = batch ? std::max(1u, std::min(cap, ctx->frame_stack_frames)) : 1;  // (no stack at all: per frame)
  return HRT_OK;
}

// One trace launch of the nf frames from frame0 (u32, wrapping like the per-frame loop's pushes);
// *stack: where it left them -- the frame stack, or lane 0's image for a single frame.
hrt_status launch_batch(hrt_context* ctx, const Batch& b, uint32_t frame0, uint32_t nf, const char** stack,
                        const hrt::MaskedPlan* masked = nullptr) {
  hrt::Lane& lane = ctx->lane[0];
  hrt::TraceParams q = b.p;
  q.pc.rng_offset = frame0;
  q.n_frames = nf;
  q.plan_valid = lane.plan_valid ? 1u : 0u;
  if (nf > 1) set_image(q, ctx, ctx->frame_stack);
  *stack = static_cast<const char*>(nf > 1 ? ctx->frame_stack : lane.trace);
  return launch_frames(ctx, q, ctx->stream, 0, masked);
}

// The trace image holds the last frame folded (frame s - 1 of a launch of nf), as after the per-frame loop.
hrt_status keep_last_frame(hrt_context* ctx, const char* stack, uint32_t nf, uint32_t s) {
  const size_t fb = ctx->npix() * ctx->px_bytes();
  if (nf > 1)
    HRT_HIP(ctx, hipMemcpyAsync(ctx->lane[0].trace, stack + (size_t)(s - 1) * fb, fb, hipMemcpyDeviceToDevice, ctx->stream));
  return HRT_OK;
}

hrt_status end_batch(hrt_context* ctx) {
  ctx->cur_lane = 0;
  ctx->cur_slot = -1;  // the trace image is lane 0's
  ctx->lane_used = true;
  return hrt::release_lane(ctx, 0);  // lane 0's next trace follows this loop
}

}  // namespace

extern "C" hrt_status hrt_compute_n(hrt_context* ctx, const hrt_push_constants* pc, uint32_t n) {
  if (!ctx || !pc) return HRT_ERR_INVALID_ARGUMENT;
  if (pc->init) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_compute_n: init dispatches go through hrt_trace");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if ((st = check_dispatch(ctx, pc, "hrt_compute_n")) != HRT_OK) return st;
  if (n == 0) return HRT_OK;
  Batch b;
  if ((st = begin_batch(ctx, pc, n, UINT32_MAX, &b)) != HRT_OK) return st;
  for (uint32_t done = 0; done < n;) {
    // near-equal launches: ceil(remaining / lcap) of them
    const uint32_t left = n - done, launches = (left + b.lcap - 1) / b.lcap;
    const uint32_t nf = (left + launches - 1) / launches, frame0 = pc->rng_offset + done;
    const char* stack = nullptr;
    if ((st = launch_batch(ctx, b, frame0, nf, &stack)) != HRT_OK) return st;
    // DiffusePipeline::next_frame(frame) for each frame, in frame order: one pass over the stack
    if ((st = hrt::fold_frames(ctx, stack, nf, frame0)) != HRT_OK) return st;
    ctx->accumulates += nf;
    if ((st = keep_last_frame(ctx, stack, nf, nf)) != HRT_OK) return st;
    done += nf;
  }
  return end_batch(ctx);
}

// hrt_compute_n's loop with a count pass between a launch's trace and its fold: the count pass runs the fold
// chain over the launch's frames in registers and writes one record per frame into the scratch ring; the
// host reads them (the call blocks here), extends the quiet run and folds only the frames up to the stop.
extern "C" hrt_status hrt_compute_until(hrt_context* ctx, const hrt_push_constants* pc, uint32_t max_frames,
                                        const hrt_settle_rule* rule, uint32_t* frames_done, uint32_t* settled) {
  if (!ctx || !pc) return HRT_ERR_INVALID_ARGUMENT;
  if (!rule || !frames_done)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_compute_until: rule and frames_done must not be NULL");
  if (rule->flags != 0) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_compute_until: rule flags must be 0");
  if (rule->quiet_frames == 0)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_compute_until: rule quiet_frames must be at least 1");
  if (pc->init) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_compute_until: init dispatches go through hrt_trace");
  if (ctx->comm)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT,
                "hrt_compute_until: the context is joined to a communicator: a group-wide rule is not supported");
  if (ctx->part_count > 1)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT,
                "hrt_compute_until: a context of a row-tile partition (part_count > 1): the parts would stop at "
                "different frames");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if ((st = check_dispatch(ctx, pc, "hrt_compute_until")) != HRT_OK) return st;
  *frames_done = 0;
  if (settled) *settled = 0;
  if (max_frames == 0) return HRT_OK;
  if (!ctx->fold_scratch)
    HRT_HIP(ctx, hrt::dev_alloc(ctx, (void**)&ctx->fold_scratch, HRT_FOLD_RECORD_RING * sizeof(hrt_fold_record)));
  Batch b;  // (a launch's frames have a slot of the scratch ring each)
  if ((st = begin_batch(ctx, pc, max_frames, HRT_FOLD_RECORD_RING, &b)) != HRT_OK) return st;
  std::vector<hrt_fold_record> recs(b.lcap);
  uint32_t done = 0, quiet_run = 0;
  bool stop = false;
  while (done < max_frames && !stop) {
    // greedy launches: whole launches until the stop
    const uint32_t nf = std::min(b.lcap, max_frames - done), frame0 = pc->rng_offset + done;
    const char* stack = nullptr;
    if ((st = launch_batch(ctx, b, frame0, nf, &stack)) != HRT_OK) return st;
    // the count pass, and its records on the host
    HRT_HIP(ctx, hipMemsetAsync(ctx->fold_scratch, 0, (size_t)nf * sizeof(hrt_fold_record), ctx->stream));
    HRT_HIP(ctx, hrt::launch_fold_records(ctx->accum, stack, ctx->f32(), ctx->npix(), ctx->real_pix(), nf, frame0, false,
                                          ctx->fold_scratch, 0, ctx->num_cus, ctx->stream));
    HRT_HIP(ctx, hipMemcpyAsync(recs.data(), ctx->fold_scratch, (size_t)nf * sizeof(hrt_fold_record),
                                hipMemcpyDeviceToHost, ctx->stream));
    HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t s = nf;  // frames of this launch to fold
    for (uint32_t f = 0; f < nf; ++f) {
      const bool quiet = recs[f].changed_pixels <= rule->max_changed_pixels && recs[f].max_delta <= rule->max_delta;
      quiet_run = quiet ? quiet_run + 1 : 0;
      if (quiet_run >= rule->quiet_frames) {
        s = f + 1;
        stop = true;
        break;
      }
    }
    // the ordinary fold of the first s frames
    if ((st = hrt::fold_frames(ctx, stack, s, frame0)) != HRT_OK) return st;
    ctx->accumulates += s;
    if ((st = keep_last_frame(ctx, stack, nf, s)) != HRT_OK) return st;
    done += s;
  }
  *frames_done = done;
  if (settled) *settled = stop ? 1u : 0u;
  return end_batch(ctx);
}

extern "C" hrt_status hrt_get_fold_records(hrt_context* ctx, hrt_fold_record* out, uint32_t cap, uint32_t* count,
                                           uint64_t* total) {
  if (!ctx || !count || (cap != 0 && !out)) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = hrt_synchronize(ctx);  // (folds the deferred combines first)
  if (st != HRT_OK) return st;
  const uint32_t ring = HRT_FOLD_RECORD_RING;
  const uint32_t n = (uint32_t)std::min<uint64_t>(cap, std::min<uint64_t>(ctx->fold_total, ring));
  if (n != 0) {
    std::vector<hrt_fold_record> all(ring);
    HRT_HIP(ctx, hipMemcpy(all.data(), ctx->fold_ring, ring * sizeof(hrt_fold_record), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t slot = (uint32_t)((ctx->fold_total - n + k) % ring);
      out[k] = all[slot];
      out[k].frame = ctx->fold_frame[slot];
      out[k].reserved = 0;
    }
  }
  *count = n;
  if (total) *total = ctx->fold_total;
  return HRT_OK;
}

extern "C" hrt_status hrt_accumulate(hrt_context* ctx, uint32_t frame) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  const int l = ctx->cur_lane;  // next_image = the most recent trace
  if (ctx->cur_slot >= 0 && ctx->defer) {
    // deferred: the next frame of a run of consecutive slots and frames, else the run is folded first
    const uint32_t s = (uint32_t)ctx->cur_slot;
    if (!ctx->pend.empty()) {
      const hrt_context::Pend& b = ctx->pend.back();
      if (!(s == b.slot + 1 && frame == b.frame + 1) && (st = hrt::flush_combines(ctx)) != HRT_OK) return st;
    }
    ctx->pend.push_back({s, frame});
    ctx->accumulates++;
    return HRT_OK;
  }
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;  // frames fold in call order
  if ((st = hrt::wait_lane(ctx, l)) != HRT_OK) return st;
  if ((st = hrt::fold_frames(ctx, hrt::trace_image(ctx), 1, frame)) != HRT_OK) return st;
  ctx->accumulates++;
  return hrt::release_lane(ctx, l);
}

namespace {

// dst <- src (npix pixels of the context's format) in format fmt, ordered on ctx->stream; blocking.
hrt_status copy_out(hrt_context* ctx, const void* src, size_t npix, uint32_t fmt, void* dst, void* scratch) {
  const size_t need = npix * (fmt == HRT_FMT_RGBA8 ? 4 : 16);
  const bool native = (ctx->mode == HRT_MODE_RGBA8) == (fmt == HRT_FMT_RGBA8);
  if (!native) {
    HRT_HIP(ctx, hrt::launch_convert(src, ctx->f32(), scratch, npix, ctx->stream));
    src = scratch;
  }
  HRT_HIP(ctx, hipMemcpyAsync(dst, src, need, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HRT_OK;
}

}  // namespace

extern "C" hrt_status hrt_read_image(hrt_context* ctx, uint32_t image_id, uint32_t fmt, void* dst, size_t bytes) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const bool local = (image_id & HRT_IMG_LOCAL) != 0;
  image_id &= ~(uint32_t)HRT_IMG_LOCAL;
  hrt_status arg = HRT_OK;
  if (image_id != HRT_IMG_TRACE && image_id != HRT_IMG_ACCUM)
    arg = fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_read_image: unknown image id");
  else if (fmt != HRT_FMT_RGBA8 && fmt != HRT_FMT_RGBA32F)
    arg = fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_read_image: unknown format");
  // the framebuffer gather: a collective, so a bad argument is agreed on by every rank, not returned here
  if (ctx->comm && !local) return hrt::comm_read_image(ctx, image_id, fmt, dst, bytes, arg);
  if (arg != HRT_OK) return arg;
  if (!dst) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_read_image: null destination");
  const size_t np = ctx->npix();
  if (bytes < np * (fmt == HRT_FMT_RGBA8 ? 4 : 16))
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_read_image: destination too small");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  const void* src = hrt::local_image(ctx, image_id);
  if (!src) return fail(ctx, HRT_ERR_HIP, "hrt_read_image: lane wait failed");
  if ((st = copy_out(ctx, src, np, fmt, dst, ctx->scratch)) != HRT_OK) return st;
  return image_id == HRT_IMG_TRACE ? hrt::release_lane(ctx, ctx->cur_lane) : HRT_OK;
}

// Checkpoint / resume: the accumulator is the whole state of a progressive render
// besides the frame counter (frame k traces with rng_offset = k), so restoring the bytes
// hrt_read_image(HRT_IMG_ACCUM) returned -- in the context's own format, no conversion -- and
// continuing with the saved frame number renders exactly what an uninterrupted run would.
extern "C" hrt_status hrt_load_accumulator(hrt_context* ctx, uint32_t fmt, const void* src, size_t bytes) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const uint32_t native = ctx->f32() ? HRT_FMT_RGBA32F : HRT_FMT_RGBA8;
  if (fmt != native)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_load_accumulator: format must be the context's own (no conversion)");
  if (!src) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_load_accumulator: null source");
  const size_t need = ctx->npix() * (fmt == HRT_FMT_RGBA8 ? 4 : 16);
  if (bytes != need) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_load_accumulator: size differs from the local image");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;  // (overwritten below, but in call order)
  if ((st = sync_all(ctx)) != HRT_OK) return st;  // no accumulate in flight
  // on the context stream (non-blocking w.r.t. the null stream): the next hrt_accumulate follows it
  HRT_HIP(ctx, hipMemcpyAsync(ctx->accum, src, need, hipMemcpyDefault, ctx->stream));  // host or device source
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HRT_OK;
}

namespace hrt {
hrt_status copy_frame_out(hrt_context* ctx, const void* src, size_t npix, uint32_t fmt, void* dst, void* scratch) {
  return copy_out(ctx, src, npix, fmt, dst, scratch);
}
}  // namespace hrt

// ---- the present pass (RenderPassOverFrame::render, src/texture_draw_pipeline.rs:96-157) ------------
namespace {

constexpr uint32_t kPresentMaxDim = 16384;

// Whether a kernel of this context may write [dst, dst + bytes): the range lies inside one of the
// context's imports, or its first and last byte are device memory of the context's device, managed
// memory or registered (pinned) host memory.  Pageable host memory is not: with XNACK off a kernel's
// store to it is a GPU fault, not an error code, so it has to be refused here.
bool present_writable(hrt_context* ctx, const void* dst, uint64_t bytes) {
  const uintptr_t a = (uintptr_t)dst;
  if (bytes == 0 || bytes - 1 > UINTPTR_MAX - a) return false;
  for (const auto& im : ctx->imports) {
    const uintptr_t b = (uintptr_t)im.ptr;
    if (a >= b && bytes <= im.bytes && a - b <= im.bytes - bytes) return true;
  }
  for (const uint64_t off : {(uint64_t)0, bytes - 1}) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, static_cast<const char*>(dst) + off) != hipSuccess) {
      (void)hipGetLastError();  // (an unknown pointer is not a sticky error)
      return false;
    }
    const bool ok = (at.type == hipMemoryTypeDevice && at.device == ctx->device) || at.type == hipMemoryTypeManaged ||
                    at.type == hipMemoryTypeHost;
    if (!ok) return false;
  }
  return true;
}

// Every argument check of hrt_present / hrt_accumulate_present, on the host, before anything is enqueued.
hrt_status check_present(hrt_context* ctx, const hrt_present_info* info, const void* dst, uint64_t dst_bytes,
                         const uint64_t* ticket, bool accum_only, const char* who) {
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  if (!info || !dst || !ticket) return bad("null info, destination or ticket");
  // a communicator: only the root of an intact hrt_comm_init_all group presents (the gathered frame)
  if (ctx->comm) {
    if (hrt_status st = hrt::comm_present_check(ctx, who); st != HRT_OK) return st;
  } else if (ctx->part_count > 1) {
    return bad("a partitioned context with no communicator cannot present (its rows are not a frame: join an "
               "hrt_comm_init_all group and present on its root)");
  }
  if (info->image_id != HRT_IMG_ACCUM && (accum_only || info->image_id != HRT_IMG_TRACE))
    return bad(accum_only ? "image_id must be HRT_IMG_ACCUM" : "unknown image id");
  if (info->format != HRT_PRESENT_B8G8R8A8 && info->format != HRT_PRESENT_R8G8B8A8) return bad("unknown present format");
  if (info->flags != 0) return bad("flags must be 0");
  if (info->width == 0 || info->height == 0 || info->width > kPresentMaxDim || info->height > kPresentMaxDim)
    return bad("target width / height must be 1..16384");
  if (info->pitch % 4 != 0 || (uint64_t)info->pitch < (uint64_t)info->width * 4)
    return bad("pitch must be a multiple of 4 and at least width * 4");
  if ((uintptr_t)dst % 4 != 0) return bad("destination must be 4-byte aligned");
  const uint64_t need = (uint64_t)(info->height - 1) * info->pitch + (uint64_t)info->width * 4;
  if (dst_bytes < need) return bad("destination smaller than (height - 1) * pitch + width * 4");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if (!present_writable(ctx, dst, need))
    return bad("destination is not an import of this context nor device, managed or registered host memory");
  return HRT_OK;
}

// The event of the next ticket: created on first use; when all kPresentRing tickets before it may still
// be in flight, the oldest (whose event this is) is waited for first.
hrt_status ticket_begin(hrt_context* ctx, hipEvent_t* ev) {
  hipEvent_t& e = ctx->present_ev[ctx->present_issued % hrt_context::kPresentRing];
  if (!e)
    HRT_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  else
    HRT_HIP(ctx, hipEventSynchronize(e));
  *ev = e;
  return HRT_OK;
}

hrt_status ticket_end(hrt_context* ctx, hipEvent_t ev, uint64_t* ticket) {
  HRT_HIP(ctx, hipEventRecord(ev, ctx->stream));
  *ticket = ++ctx->present_issued;
  return HRT_OK;
}

hrt::PresentTarget present_target(const hrt_present_info* info, void* dst) {
  return {static_cast<unsigned char*>(dst), info->width, info->height, info->pitch,
          info->format == HRT_PRESENT_B8G8R8A8 ? 1u : 0u};
}

// The pass itself on ctx->stream, after everything that wrote the image (arguments already checked).
hrt_status enqueue_present(hrt_context* ctx, const hrt_present_info* info, void* dst) {
  // the root of a group (check_present let no other communicator through): the gathered frame
  if (ctx->comm) return hrt::comm_present(ctx, info->image_id, present_target(info, dst));
  const void* src = hrt::local_image(ctx, info->image_id);
  if (!src) return fail(ctx, HRT_ERR_HIP, "hrt_present: lane wait failed");
  HRT_HIP(ctx, hrt::launch_present(src, ctx->f32(), ctx->width, ctx->local_rows, present_target(info, dst), ctx->stream));
  if (info->image_id != HRT_IMG_TRACE) return HRT_OK;
  // the trace image's next writer follows the pass: its lane's next trace, and -- when the image is a
  // slot of the deferred combiner's ring -- the slot's next trace, which waits for fold_done
  if (ctx->cur_slot >= 0) {
    HRT_HIP(ctx, hipEventRecord(ctx->fold_done, ctx->stream));
    ctx->fold_set = true;
  }
  return hrt::release_lane(ctx, ctx->cur_lane);
}

}  // namespace

extern "C" hrt_status hrt_present(hrt_context* ctx, const hrt_present_info* info, void* dst, uint64_t dst_bytes,
                                  uint64_t* ticket) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = check_present(ctx, info, dst, dst_bytes, ticket, false, "hrt_present");
  if (st != HRT_OK) return st;
  hipEvent_t ev = nullptr;
  if ((st = ticket_begin(ctx, &ev)) != HRT_OK) return st;
  if ((st = enqueue_present(ctx, info, dst)) != HRT_OK) return st;
  return ticket_end(ctx, ev, ticket);
}

extern "C" hrt_status hrt_accumulate_present(hrt_context* ctx, uint32_t frame, const hrt_present_info* info, void* dst,
                                             uint64_t dst_bytes, uint64_t* ticket) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = check_present(ctx, info, dst, dst_bytes, ticket, true, "hrt_accumulate_present");
  if (st != HRT_OK) return st;
  hipEvent_t ev = nullptr;
  if ((st = ticket_begin(ctx, &ev)) != HRT_OK) return st;
  if (const std::vector<hrt_context*>* members = hrt::comm_group_members(ctx)) {
    // the root of a group: every part folds its own rows on its own device and stream, in part order,
    // then the gathered present of the accumulator (no fused kernel: the fold and the target are on
    // different contexts)
    for (hrt_context* m : *members)
      if ((st = hrt_accumulate(m, frame)) != HRT_OK) {
        if (m != ctx) ctx->err = m->err;
        (void)bind(ctx);
        return st;
      }
    if ((st = enqueue_present(ctx, info, dst)) != HRT_OK) return st;
    return ticket_end(ctx, ev, ticket);
  }
  if (ctx->defer || ctx->fold_on || info->width != ctx->width || info->height != ctx->local_rows) {
    // the two passes: a deferred combine is folded by the present, a scaled target samples the new accumulator,
    // a recorded fold (HRT_OPT_FOLD_RECORDS) is the recording combiner's
    if ((st = hrt_accumulate(ctx, frame)) != HRT_OK) return st;
    if ((st = enqueue_present(ctx, info, dst)) != HRT_OK) return st;
    return ticket_end(ctx, ev, ticket);
  }
  // hrt_accumulate's immediate combine with the target's pixel written by the same kernel
  const int l = ctx->cur_lane;
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;
  if ((st = hrt::wait_lane(ctx, l)) != HRT_OK) return st;
  HRT_HIP(ctx, hrt::launch_accumulate_present(ctx->accum, hrt::trace_image(ctx), ctx->f32(), ctx->width, ctx->local_rows,
                                              frame, present_target(info, dst), ctx->stream));
  ctx->accumulates++;
  if ((st = hrt::release_lane(ctx, l)) != HRT_OK) return st;
  return ticket_end(ctx, ev, ticket);
}

// ---- the denoise pass (kernels in hrt_denoise.hip) ---------------------------
namespace {

// Every check of hrt_denoise / hrt_denoise_present that concerns the filter itself, on the host.
hrt_status check_denoise(hrt_context* ctx, const hrt_denoise_info* info, const hrt_hit* guide, const char* who) {
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  if (!info) return bad("null info");
  if (ctx->comm || ctx->part_count > 1)
    return bad("a context of a row-tile partition or joined to a communicator cannot denoise (a tap's neighbour rows "
               "live on another part; the gathered form is out of scope)");
  if (info->image_id != HRT_IMG_ACCUM && info->image_id != HRT_IMG_TRACE) return bad("unknown image id");
  if (info->iterations == 0 || info->iterations > hrt::kDenoiseMaxIterations) return bad("iterations must be 1..5");
#ifdef HRT_DEBUG_OPTIONS
  if (info->method > HRT_DEBUG_DENOISE_LATTICE) return bad("unknown method");
#else
  if (info->method > HRT_DENOISE_TILED) return bad("unknown method");
#endif
  if (info->flags != 0) return bad("flags must be 0");
  for (const float s : {info->sigma_colour, info->sigma_normal, info->sigma_depth})
    if (!(std::isfinite(s) && s > 0.0f)) return bad("every sigma must be finite and greater than 0");
  if (guide) {
    hrt_status st = bind(ctx);
    if (st != HRT_OK) return st;
    if ((uintptr_t)guide % 16 != 0) return bad("the guide must be 16-byte aligned");
    if (!query_direct(ctx, guide) || !query_direct(ctx, guide + (ctx->npix() - 1)))
      return bad("the guide must be width x height records in memory of the context's device");
  }
  return HRT_OK;
}

// The filter on ctx->stream, after everything that wrote the source image (arguments already checked): prep,
// then one pass per iteration between the two scratch images.  The last pass writes out (float4 texels, or
// RGBA8 words when out_rgba8) when out is not null, else the scratch image the pass before it did not write;
// *result = where the result is.
hrt_status enqueue_denoise(hrt_context* ctx, const hrt_denoise_info* info, const hrt_hit* guide, void* out, bool out_rgba8,
                           void** result, const char* who) {
  const size_t np = ctx->npix();
  hrt_status st;
  for (void*& img : ctx->dn_img)
    if ((st = ensure_staging(ctx, &img, np * 16, who)) != HRT_OK) return st;
  if (guide) {
    if ((st = ensure_staging(ctx, &ctx->dn_guide, np * 16, who)) != HRT_OK) return st;
    if ((st = ensure_staging(ctx, &ctx->dn_keys, np * 4, who)) != HRT_OK) return st;
  }
  void* gd = guide ? ctx->dn_guide : nullptr;
  void* keys = guide ? ctx->dn_keys : nullptr;
  const void* src = hrt::local_image(ctx, info->image_id);
  if (!src) return fail(ctx, HRT_ERR_HIP, std::string(who) + ": lane wait failed");
  HRT_HIP(ctx, hrt::launch_denoise_prep(src, ctx->f32(), guide, ctx->dn_img[0], gd, keys, np, ctx->stream));
  if (info->image_id == HRT_IMG_TRACE) {
    // prep was the source's only reader: the trace image's next writer follows it (enqueue_present's rule)
    if (ctx->cur_slot >= 0) {
      HRT_HIP(ctx, hipEventRecord(ctx->fold_done, ctx->stream));
      ctx->fold_set = true;
    }
    if ((st = hrt::release_lane(ctx, ctx->cur_lane)) != HRT_OK) return st;
  }
  // S14's host constants, each one rounded float operation
  const float kc0 = 1.0f / (info->sigma_colour * info->sigma_colour), kn = 1.0f / info->sigma_normal;
  for (uint32_t i = 0; i < info->iterations; ++i) {
    const bool last = i + 1 == info->iterations;
    void* to = last && out ? out : ctx->dn_img[(i + 1) & 1];
    const hrt::AtrousPass p{ctx->dn_img[i & 1], gd, keys, to, last && out_rgba8, ctx->width, ctx->local_rows, 1u << i,
                            ldexpf(kc0, 2 * (int)i), kn, info->sigma_depth};
    HRT_HIP(ctx, hrt::launch_atrous(p, hrt::atrous_form(info->method, i), ctx->stream));
    *result = to;
  }
  return HRT_OK;
}

}  // namespace

extern "C" void hrt_denoise_defaults(hrt_denoise_info* info) {
  if (!info) return;
  *info = hrt_denoise_info{HRT_IMG_ACCUM, hrt::kDenoiseMaxIterations, HRT_DENOISE_AUTO, 0u,
                           HRT_DENOISE_SIGMA_COLOUR, HRT_DENOISE_SIGMA_NORMAL, HRT_DENOISE_SIGMA_DEPTH, 0u};
}

extern "C" hrt_status hrt_denoise(hrt_context* ctx, const hrt_denoise_info* info, const hrt_hit* guide, uint32_t fmt,
                                  void* dst, size_t bytes) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = check_denoise(ctx, info, guide, "hrt_denoise");
  if (st != HRT_OK) return st;
  if (fmt != HRT_FMT_RGBA8 && fmt != HRT_FMT_RGBA32F) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_denoise: unknown format");
  if (!dst) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_denoise: null destination");
  const bool rgba8 = fmt == HRT_FMT_RGBA8;
  const size_t need = ctx->npix() * (rgba8 ? 4 : 16);
  if (bytes < need) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_denoise: destination too small");
  if ((st = bind(ctx)) != HRT_OK) return st;
  // device memory a texel store may address: the last pass writes it; anything else is copied from the scratch
  const bool direct = (uintptr_t)dst % (rgba8 ? 4 : 16) == 0 && query_direct(ctx, dst) &&
                      query_direct(ctx, static_cast<const char*>(dst) + (need - 1));
  void* res = nullptr;
  if ((st = enqueue_denoise(ctx, info, guide, direct ? dst : nullptr, rgba8, &res, "hrt_denoise")) != HRT_OK) return st;
  if (!direct) HRT_HIP(ctx, hipMemcpyAsync(dst, res, need, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HRT_OK;
}

extern "C" hrt_status hrt_denoise_present(hrt_context* ctx, const hrt_denoise_info* info, const hrt_hit* guide,
                                          const hrt_present_info* target, void* dst, uint64_t dst_bytes,
                                          uint64_t* ticket) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = check_denoise(ctx, info, guide, "hrt_denoise_present");
  if (st != HRT_OK) return st;
  if ((st = check_present(ctx, target, dst, dst_bytes, ticket, false, "hrt_denoise_present")) != HRT_OK) return st;
  if (target->image_id != info->image_id)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_denoise_present: the target's image_id differs from the filter's");
  hipEvent_t ev = nullptr;
  if ((st = ticket_begin(ctx, &ev)) != HRT_OK) return st;
  void* res = nullptr;
  if ((st = enqueue_denoise(ctx, info, guide, nullptr, false, &res, "hrt_denoise_present")) != HRT_OK) return st;
  // the filtered float image through the present pass unchanged
  HRT_HIP(ctx, hrt::launch_present(res, true, ctx->width, ctx->local_rows, present_target(target, dst), ctx->stream));
  return ticket_end(ctx, ev, ticket);
}

// ---- temporal history (kernels in hrt_history.hip) -----------------------------
namespace {

// What all four history calls refuse, and the count image: allocated and zeroed (on ctx->stream) by the first.
hrt_status begin_history(hrt_context* ctx, const char* who) {
  if (ctx->comm || ctx->part_count > 1)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT,
                std::string(who) + ": a context of a row-tile partition or joined to a communicator keeps no history (a "
                                   "reprojected pixel's source rows live on another part; the gathered form is out of scope)");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if (ctx->hist_cnt) return HRT_OK;
  void* p = nullptr;
  if ((st = ensure_staging(ctx, &p, ctx->npix() * 4, who)) != HRT_OK) return st;
  ctx->hist_cnt = static_cast<uint32_t*>(p);
  HRT_HIP(ctx, hipMemsetAsync(ctx->hist_cnt, 0, ctx->npix() * 4, ctx->stream));
  return HRT_OK;
}

// The moments image of the variance-guided denoise (S16): allocated and zeroed (on ctx->stream) by the first call
// that needs it, after begin_history's refusals.
hrt_status begin_moments(hrt_context* ctx, const char* who) {
  if (ctx->hist_mom) return HRT_OK;
  void* p = nullptr;
  hrt_status st = ensure_staging(ctx, &p, ctx->npix() * 8, who);
  if (st != HRT_OK) return st;
  ctx->hist_mom = static_cast<float*>(p);
  HRT_HIP(ctx, hipMemsetAsync(ctx->hist_mom, 0, ctx->npix() * 8, ctx->stream));
  return HRT_OK;
}

bool hits_on_device(hrt_context* ctx, const hrt_hit* hits) {
  return query_direct(ctx, hits) && query_direct(ctx, hits + (ctx->npix() - 1));
}

}  // namespace

extern "C" void hrt_reproject_defaults(hrt_reproject_info* info) {
  if (!info) return;
  *info = hrt_reproject_info{HRT_REPROJECT_BILINEAR, 0u, HRT_REPROJECT_DEPTH_TOLERANCE, HRT_REPROJECT_MIN_NORMAL_DOT,
                             {0u, 0u, 0u, 0u}};
}

namespace {

// The new rejections of hrt_reproject_motion[_moments] (host only): the reason, or null.  *moving: whether any entry
// has HRT_MOTION_MOVING.
const char* check_motion(const hrt_motion_tables* m, bool* moving) {
  if (m->n_spheres > HRT_MOTION_MAX_OBJECTS || m->n_meshes > HRT_MOTION_MAX_OBJECTS)
    return "a motion table holds more than HRT_MOTION_MAX_OBJECTS entries";
  if ((m->n_spheres && !m->spheres) || (m->n_meshes && !m->meshes)) return "a motion table with a count has a null pointer";
  const hrt_motion* tab[2] = {m->spheres, m->meshes};
  const uint32_t n[2] = {m->n_spheres, m->n_meshes};
  for (int t = 0; t < 2; ++t)
    for (uint32_t i = 0; i < n[t]; ++i) {
      const hrt_motion& e = tab[t][i];
      if (e.flags & ~HRT_MOTION_MOVING) return "a motion entry has an unknown flag bit";
      if (!(e.flags & HRT_MOTION_MOVING)) continue;
      *moving = true;
      for (float v : e.m)
        if (!std::isfinite(v)) return "a moving motion entry has a component that is not finite";
    }
  return nullptr;
}

// Copies the caller's tables into the next slot of the context's ring and enqueues the slot's upload on ctx->stream;
// *tabs = the device tables the pass reads.  Blocks only for the slot's previous pass (the ring is exhausted) --
// the caller records slot->done once more after its pass.
hrt_status stage_motion(hrt_context* ctx, const hrt_motion_tables* m, hrt_context::MotionSlot** out, hrt::MotionTables* tabs,
                        const char* who) {
  hrt_context::MotionSlot& s = ctx->motion_ring[ctx->motion_next];
  const size_t sb = (size_t)m->n_spheres * sizeof(hrt_motion), mb = (size_t)m->n_meshes * sizeof(hrt_motion);
  const size_t need = sb + mb;  // (not 0: an entry moves)
  if (!s.done) HRT_HIP(ctx, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  if (s.used) HRT_HIP(ctx, hipEventSynchronize(s.done));
  s.used = false;
  if (s.bytes < need) {  // (the slot's last pass has run: nothing reads the old buffers)
    if (s.host) (void)hipHostFree(s.host);
    free_dev(ctx, s.dev);
    s.host = nullptr;
    s.bytes = 0;
    if (hipHostMalloc(&s.host, need, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      s.host = nullptr;
      return fail(ctx, HRT_ERR_OUT_OF_MEMORY, std::string(who) + ": pinned staging allocation failed");
    }
    hrt_status st = ensure_staging(ctx, &s.dev, need, who);
    if (st != HRT_OK) {
      (void)hipHostFree(s.host);
      s.host = nullptr;
      return st;
    }
    s.bytes = need;
  }
  if (sb) std::memcpy(s.host, m->spheres, sb);
  if (mb) std::memcpy(static_cast<char*>(s.host) + sb, m->meshes, mb);
  HRT_HIP(ctx, hipMemcpyAsync(s.dev, s.host, need, hipMemcpyHostToDevice, ctx->stream));
  // from here on the slot's buffers are in use: should the pass after this not be enqueued, the slot's next user
  // still waits for the upload (the caller records the event once more behind its pass)
  s.used = true;
  HRT_HIP(ctx, hipEventRecord(s.done, ctx->stream));
  tabs->spheres = m->n_spheres ? static_cast<const hrt_motion*>(s.dev) : nullptr;
  tabs->meshes = m->n_meshes ? reinterpret_cast<const hrt_motion*>(static_cast<const char*>(s.dev) + sb) : nullptr;
  tabs->n_spheres = m->n_spheres;
  tabs->n_meshes = m->n_meshes;
  ctx->motion_next = (ctx->motion_next + 1u) % HRT_MOTION_RING;
  *out = &s;
  return HRT_OK;
}

// hrt_reproject (moments false) and hrt_reproject_moments: the same checks, order and swaps; with moments the pass
// also writes M' into hist_mom_next, swapped with hist_mom like the other two.
// with_motion: hrt_reproject_motion[_moments] -- the tables are checked with the other arguments, staged through the
// context's ring (stage_motion) after everything that can still refuse, and the motion form of the pass runs; a
// call none of whose entries moves runs the plain pass, whose bytes S21 makes its own.
hrt_status reproject_call(hrt_context* ctx, const hrt_reproject_info* info, const hrt_view* prev, const hrt_hit* prev_hits,
                          const hrt_view* cur, const hrt_hit* cur_hits, bool moments, const char* who,
                          bool with_motion = false, const hrt_motion_tables* motion = nullptr) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  if (!info) return bad("null info");
  if (!prev || !cur) return bad("null view");
  if (!prev_hits || !cur_hits) return bad("null hit array");
  if (info->filter != HRT_REPROJECT_NEAREST && info->filter != HRT_REPROJECT_BILINEAR) return bad("unknown filter");
  if (info->flags != 0) return bad("flags must be 0");
  if (!(std::isfinite(info->depth_tolerance) && info->depth_tolerance >= 0.0f))
    return bad("depth_tolerance must be finite and not negative");
  if (!std::isfinite(info->min_normal_dot)) return bad("min_normal_dot must be finite");
  bool moving = false;
  if (with_motion) {
    if (!motion) return bad("null motion tables");
    if (const char* why = check_motion(motion, &moving)) return bad(why);
  }
  if (ctx->comm || ctx->part_count > 1) return begin_history(ctx, who);  // (the rejection)
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if ((uintptr_t)prev_hits % 16 != 0 || (uintptr_t)cur_hits % 16 != 0) return bad("the hit arrays must be 16-byte aligned");
  if (!hits_on_device(ctx, prev_hits) || !hits_on_device(ctx, cur_hits))
    return bad("the hit arrays must be width x height records in memory of the context's device");
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;
  if ((st = begin_history(ctx, who)) != HRT_OK) return st;
  const size_t np = ctx->npix();
  void* p = ctx->hist_cnt_next;
  if ((st = ensure_staging(ctx, &p, np * 4, who)) != HRT_OK) return st;
  ctx->hist_cnt_next = static_cast<uint32_t*>(p);
  if ((st = ensure_staging(ctx, &ctx->hist_accum_next, np * ctx->px_bytes(), who)) != HRT_OK) return st;
  if (moments) {
    if ((st = begin_moments(ctx, who)) != HRT_OK) return st;
    p = ctx->hist_mom_next;
    if ((st = ensure_staging(ctx, &p, np * 8, who)) != HRT_OK) return st;
    ctx->hist_mom_next = static_cast<float*>(p);
  }
  const hrt::ReprojectPass pass{ctx->accum, ctx->hist_cnt, ctx->hist_accum_next, ctx->hist_cnt_next, prev_hits, cur_hits,
                                *prev, *cur, ctx->f32(), info->filter, ctx->width, ctx->local_rows,
                                info->depth_tolerance, info->min_normal_dot};
  if (moving) {
    hrt_context::MotionSlot* slot = nullptr;
    hrt::MotionTables tabs{};
    if ((st = stage_motion(ctx, motion, &slot, &tabs, who)) != HRT_OK) return st;
    HRT_HIP(ctx, hrt::launch_reproject_motion(pass, tabs, moments ? ctx->hist_mom : nullptr,
                                              moments ? ctx->hist_mom_next : nullptr, ctx->stream));
    HRT_HIP(ctx, hipEventRecord(slot->done, ctx->stream));  // the slot's next user waits for the pass
  } else if (moments) {
    HRT_HIP(ctx, hrt::launch_reproject_moments(pass, ctx->hist_mom, ctx->hist_mom_next, ctx->stream));
  } else {
    HRT_HIP(ctx, hrt::launch_reproject(pass, ctx->stream));
  }
  // A' and N' become the context's accumulator and count image; the old ones are the next pass's targets
  std::swap(ctx->accum, ctx->hist_accum_next);
  std::swap(ctx->hist_cnt, ctx->hist_cnt_next);
  if (moments) std::swap(ctx->hist_mom, ctx->hist_mom_next);
  return HRT_OK;
}

// hrt_accumulate_history (moments false) and hrt_accumulate_history_moments.
hrt_status accumulate_history_call(hrt_context* ctx, uint32_t max_history, bool moments, const char* who) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  if (max_history == 0 || max_history > hrt::kHistoryMax)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": max_history must be 1..2^24");
  hrt_status st = begin_history(ctx, who);
  if (st != HRT_OK) return st;
  if (moments && (st = begin_moments(ctx, who)) != HRT_OK) return st;
  const int l = ctx->cur_lane;  // next_image = the most recent trace
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;  // frames fold in call order
  if ((st = hrt::wait_lane(ctx, l)) != HRT_OK) return st;
  if (moments)
    HRT_HIP(ctx, hrt::launch_fold_history_moments(ctx->accum, hrt::trace_image(ctx), ctx->hist_cnt, ctx->hist_mom, ctx->f32(),
                                                  ctx->npix(), max_history, ctx->stream));
  else
    HRT_HIP(ctx, hrt::launch_fold_history(ctx->accum, hrt::trace_image(ctx), ctx->hist_cnt, ctx->f32(), ctx->npix(),
                                          max_history, ctx->stream));
  if (ctx->cur_slot >= 0) {  // a slot of the deferred combiner's ring: its next trace waits for this fold
    HRT_HIP(ctx, hipEventRecord(ctx->fold_done, ctx->stream));
    ctx->fold_set = true;
  }
  ctx->accumulates++;
  return hrt::release_lane(ctx, l);
}

}  // namespace

extern "C" hrt_status hrt_reproject(hrt_context* ctx, const hrt_reproject_info* info, const hrt_view* prev,
                                    const hrt_hit* prev_hits, const hrt_view* cur, const hrt_hit* cur_hits) {
  return reproject_call(ctx, info, prev, prev_hits, cur, cur_hits, false, "hrt_reproject");
}

extern "C" hrt_status hrt_accumulate_history(hrt_context* ctx, uint32_t max_history) {
  return accumulate_history_call(ctx, max_history, false, "hrt_accumulate_history");
}

extern "C" hrt_status hrt_fill_history(hrt_context* ctx, uint32_t count) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = begin_history(ctx, "hrt_fill_history");
  if (st != HRT_OK) return st;
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;
  HRT_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->hist_cnt, (int)count, ctx->npix(), ctx->stream));
  return HRT_OK;
}

extern "C" hrt_status hrt_read_history(hrt_context* ctx, uint32_t* dst, size_t bytes) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  if (!dst) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_read_history: null destination");
  const size_t need = ctx->npix() * 4;
  if (bytes < need) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_read_history: destination too small");
  hrt_status st = begin_history(ctx, "hrt_read_history");
  if (st != HRT_OK) return st;
  HRT_HIP(ctx, hipMemcpyAsync(dst, ctx->hist_cnt, need, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HRT_OK;
}

// ---- the variance-guided denoise (kernels in hrt_variance.hip and hrt_history.hip) -----
extern "C" hrt_status hrt_accumulate_history_moments(hrt_context* ctx, uint32_t max_history) {
  return accumulate_history_call(ctx, max_history, true, "hrt_accumulate_history_moments");
}

extern "C" hrt_status hrt_reproject_moments(hrt_context* ctx, const hrt_reproject_info* info, const hrt_view* prev,
                                            const hrt_hit* prev_hits, const hrt_view* cur, const hrt_hit* cur_hits) {
  return reproject_call(ctx, info, prev, prev_hits, cur, cur_hits, true, "hrt_reproject_moments");
}

// ---- object motion in the temporal history (the motion forms in hrt_history.hip) -------
extern "C" hrt_status hrt_reproject_motion(hrt_context* ctx, const hrt_reproject_info* info, const hrt_motion_tables* motion,
                                           const hrt_view* prev, const hrt_hit* prev_hits, const hrt_view* cur,
                                           const hrt_hit* cur_hits) {
  return reproject_call(ctx, info, prev, prev_hits, cur, cur_hits, false, "hrt_reproject_motion", true, motion);
}

extern "C" hrt_status hrt_reproject_motion_moments(hrt_context* ctx, const hrt_reproject_info* info,
                                                   const hrt_motion_tables* motion, const hrt_view* prev,
                                                   const hrt_hit* prev_hits, const hrt_view* cur, const hrt_hit* cur_hits) {
  return reproject_call(ctx, info, prev, prev_hits, cur, cur_hits, true, "hrt_reproject_motion_moments", true, motion);
}

extern "C" hrt_status hrt_fill_moments(hrt_context* ctx, float m1, float m2) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = begin_history(ctx, "hrt_fill_moments");
  if (st != HRT_OK) return st;
  if ((st = begin_moments(ctx, "hrt_fill_moments")) != HRT_OK) return st;
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;
  HRT_HIP(ctx, hrt::launch_fill_moments(ctx->hist_mom, ctx->npix(), m1, m2, ctx->stream));
  return HRT_OK;
}

extern "C" hrt_status hrt_read_moments(hrt_context* ctx, float* dst, size_t bytes) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  if (!dst) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_read_moments: null destination");
  const size_t need = ctx->npix() * 8;
  if (bytes < need) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_read_moments: destination too small");
  hrt_status st = begin_history(ctx, "hrt_read_moments");
  if (st != HRT_OK) return st;
  if ((st = begin_moments(ctx, "hrt_read_moments")) != HRT_OK) return st;
  HRT_HIP(ctx, hipMemcpyAsync(dst, ctx->hist_mom, need, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HRT_OK;
}

namespace {

// Every check of hrt_denoise_variance / hrt_denoise_variance_present that concerns the filter itself, on the host.
hrt_status check_variance(hrt_context* ctx, const hrt_variance_info* info, const hrt_hit* guide, const char* who) {
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  if (!info) return bad("null info");
  if (ctx->comm || ctx->part_count > 1)
    return bad("a context of a row-tile partition or joined to a communicator cannot denoise (a tap's neighbour rows "
               "live on another part; the gathered form is out of scope)");
  if (info->iterations > hrt::kVarianceMaxIterations) return bad("iterations must be 0..5");
  if (info->method > HRT_VARIANCE_TILED) return bad("unknown method");
  if (info->flags != 0) return bad("flags must be 0");
  if (info->min_history == 0) return bad("min_history must be at least 1");
  for (const float s : {info->sigma_variance, info->variance_floor, info->sigma_normal, info->sigma_depth})
    if (!(std::isfinite(s) && s > 0.0f)) return bad("every sigma and the variance floor must be finite and greater than 0");
  if (guide) {
    hrt_status st = bind(ctx);
    if (st != HRT_OK) return st;
    if ((uintptr_t)guide % 16 != 0) return bad("the guide must be 16-byte aligned");
    if (!query_direct(ctx, guide) || !query_direct(ctx, guide + (ctx->npix() - 1)))
      return bad("the guide must be width x height records in memory of the context's device");
  }
  return HRT_OK;
}

// The filter on ctx->stream, after everything that wrote the accumulator, N and M (arguments already checked):
// variance_prep, then one pass per iteration between hrt_denoise's two scratch images.  The last pass (with no
// iterations: variance_store) writes `out` (float4 texels, or RGBA8 words when out_rgba8) when out is not null,
// else the scratch image the pass before it did not write, and the variance to vout when that is not null;
// *result = where the image is.
hrt_status enqueue_variance(hrt_context* ctx, const hrt_variance_info* info, const hrt_hit* guide, void* out, bool out_rgba8,
                            float* vout, void** result, const char* who) {
  const size_t np = ctx->npix();
  hrt_status st;
  if ((st = begin_history(ctx, who)) != HRT_OK) return st;
  if ((st = begin_moments(ctx, who)) != HRT_OK) return st;
  for (void*& img : ctx->dn_img)
    if ((st = ensure_staging(ctx, &img, np * 16, who)) != HRT_OK) return st;
  if (guide) {
    if ((st = ensure_staging(ctx, &ctx->dn_guide, np * 16, who)) != HRT_OK) return st;
    if ((st = ensure_staging(ctx, &ctx->dn_keys, np * 4, who)) != HRT_OK) return st;
  }
  void* gd = guide ? ctx->dn_guide : nullptr;
  void* keys = guide ? ctx->dn_keys : nullptr;
  const void* src = hrt::local_image(ctx, HRT_IMG_ACCUM);
  if (!src) return fail(ctx, HRT_ERR_HIP, std::string(who) + ": lane wait failed");
  const hrt::VariancePrep prep{src, ctx->f32(), guide, ctx->hist_cnt, ctx->hist_mom, ctx->dn_img[0], gd, keys,
                               ctx->width, ctx->local_rows, info->min_history};
  HRT_HIP(ctx, hrt::launch_variance_prep(prep, ctx->stream));
  const int final_kind = out_rgba8 ? hrt::kVarianceOutRgba8 : hrt::kVarianceOutFloat;
  if (info->iterations == 0) {
    void* to = out ? out : ctx->dn_img[1];
    HRT_HIP(ctx, hrt::launch_variance_store(ctx->dn_img[0], to, vout, final_kind, np, ctx->stream));
    *result = to;
    return HRT_OK;
  }
  // S16's and S14's host constants, each one rounded float operation
  const float sv2 = info->sigma_variance * info->sigma_variance, kn = 1.0f / info->sigma_normal;
  for (uint32_t i = 0; i < info->iterations; ++i) {
    const bool last = i + 1 == info->iterations;
    void* to = last && out ? out : ctx->dn_img[(i + 1) & 1];
    const hrt::VariancePass p{ctx->dn_img[i & 1], gd, keys, to, last ? vout : nullptr, last ? final_kind : hrt::kVarianceOutPass,
                              ctx->width, ctx->local_rows, 1u << i, sv2, info->variance_floor, kn, info->sigma_depth};
    HRT_HIP(ctx, hrt::launch_variance_atrous(p, hrt::variance_form(info->method, i), ctx->stream));
    *result = to;
  }
  return HRT_OK;
}

}  // namespace

extern "C" void hrt_variance_defaults(hrt_variance_info* info) {
  if (!info) return;
  *info = hrt_variance_info{hrt::kVarianceMaxIterations, HRT_VARIANCE_AUTO, 0u, HRT_VARIANCE_MIN_HISTORY,
                            HRT_VARIANCE_SIGMA, HRT_VARIANCE_FLOOR, HRT_DENOISE_SIGMA_NORMAL, HRT_DENOISE_SIGMA_DEPTH};
}

extern "C" hrt_status hrt_denoise_variance(hrt_context* ctx, const hrt_variance_info* info, const hrt_hit* guide, uint32_t fmt,
                                           void* dst, size_t bytes, float* variance_dst, size_t variance_bytes) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_denoise_variance";
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  hrt_status st = check_variance(ctx, info, guide, who);
  if (st != HRT_OK) return st;
  if (fmt != HRT_FMT_RGBA8 && fmt != HRT_FMT_RGBA32F) return bad("unknown format");
  if (!dst) return bad("null destination");
  const bool rgba8 = fmt == HRT_FMT_RGBA8;
  const size_t need = ctx->npix() * (rgba8 ? 4 : 16), vneed = ctx->npix() * 4;
  if (bytes < need) return bad("destination too small");
  if (variance_dst && variance_bytes < vneed) return bad("variance destination too small");
  if ((st = bind(ctx)) != HRT_OK) return st;
  // device memory a store may address: the last pass writes it; anything else is copied from the scratch
  const bool direct = (uintptr_t)dst % (rgba8 ? 4 : 16) == 0 && query_direct(ctx, dst) &&
                      query_direct(ctx, static_cast<const char*>(dst) + (need - 1));
  const bool vdirect = variance_dst && (uintptr_t)variance_dst % 4 == 0 && query_direct(ctx, variance_dst) &&
                       query_direct(ctx, reinterpret_cast<const char*>(variance_dst) + (vneed - 1));
  float* vout = nullptr;
  if (variance_dst) {
    vout = variance_dst;
    if (!vdirect) {
      void* p = ctx->var_stage;
      if ((st = ensure_staging(ctx, &p, vneed, who)) != HRT_OK) return st;
      vout = ctx->var_stage = static_cast<float*>(p);
    }
  }
  void* res = nullptr;
  if ((st = enqueue_variance(ctx, info, guide, direct ? dst : nullptr, rgba8, vout, &res, who)) != HRT_OK) return st;
  if (!direct) HRT_HIP(ctx, hipMemcpyAsync(dst, res, need, hipMemcpyDefault, ctx->stream));
  if (variance_dst && !vdirect) HRT_HIP(ctx, hipMemcpyAsync(variance_dst, vout, vneed, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HRT_OK;
}

extern "C" hrt_status hrt_denoise_variance_present(hrt_context* ctx, const hrt_variance_info* info, const hrt_hit* guide,
                                                   const hrt_present_info* target, void* dst, uint64_t dst_bytes,
                                                   uint64_t* ticket) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_denoise_variance_present";
  hrt_status st = check_variance(ctx, info, guide, who);
  if (st != HRT_OK) return st;
  if ((st = check_present(ctx, target, dst, dst_bytes, ticket, true, who)) != HRT_OK) return st;
  hipEvent_t ev = nullptr;
  if ((st = ticket_begin(ctx, &ev)) != HRT_OK) return st;
  void* res = nullptr;
  if ((st = enqueue_variance(ctx, info, guide, nullptr, false, nullptr, &res, who)) != HRT_OK) return st;
  // the filtered float image through the present pass unchanged
  HRT_HIP(ctx, hrt::launch_present(res, true, ctx->width, ctx->local_rows, present_target(target, dst), ctx->stream));
  return ticket_end(ctx, ev, ticket);
}

// ---- guided upsampling (kernel in hrt_upsample.hip) ------------------------------------
namespace {

constexpr uint32_t kUpsampleMaxDim = 16384;

// Every check of hrt_upsample / hrt_upsample_present that concerns the pass itself, on the host: its own
// arguments, then the given filter's (check_denoise / check_variance with low_hits as the guide).
hrt_status check_upsample(hrt_context* ctx, const hrt_upsample_info* info, const hrt_denoise_info* denoise,
                          const hrt_variance_info* variance, const hrt_hit* low_hits, const hrt_hit* high_hits,
                          const char* who) {
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  if (!info) return bad("null info");
  if (!low_hits || !high_hits) return bad("null low_hits or high_hits");
  if (denoise && variance) return bad("at most one of denoise and variance may be given");
  if (ctx->comm || ctx->part_count > 1)
    return bad("a context of a row-tile partition or joined to a communicator cannot upsample (a tap's neighbour rows "
               "live on another part; the gathered form is out of scope)");
  if (info->image_id != HRT_IMG_ACCUM && info->image_id != HRT_IMG_TRACE) return bad("unknown image id");
  if (info->footprint != 2 && info->footprint != 4) return bad("footprint must be 2 or 4");
  if (info->flags != 0) return bad("flags must be 0");
  for (const float s : {info->sigma_normal, info->sigma_depth})
    if (!(std::isfinite(s) && s > 0.0f)) return bad("every sigma must be finite and greater than 0");
  if (info->width == 0 || info->height == 0 || info->width > kUpsampleMaxDim || info->height > kUpsampleMaxDim)
    return bad("width / height must be 1..16384");
  if (ctx->width > (1u << 24) || ctx->local_rows > (1u << 24)) return bad("the context's image is wider or taller than 2^24");
  if (denoise && denoise->image_id != info->image_id) return bad("the denoise filter's image_id differs from info's");
  if (variance && info->image_id != HRT_IMG_ACCUM) return bad("the variance filter reads the accumulator: image_id must be HRT_IMG_ACCUM");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if ((uintptr_t)low_hits % 16 != 0 || (uintptr_t)high_hits % 16 != 0) return bad("low_hits and high_hits must be 16-byte aligned");
  if (!query_direct(ctx, low_hits) || !query_direct(ctx, low_hits + (ctx->npix() - 1)))
    return bad("low_hits must be the context's width x height records in memory of the context's device");
  const size_t nt = (size_t)info->width * info->height;
  if (!query_direct(ctx, high_hits) || !query_direct(ctx, high_hits + (nt - 1)))
    return bad("high_hits must be info->width x info->height records in memory of the context's device");
  if (denoise) return check_denoise(ctx, denoise, low_hits, who);
  if (variance) return check_variance(ctx, variance, low_hits, who);
  return HRT_OK;
}

// The pass on ctx->stream, after everything that wrote the source image (arguments already checked): the given
// filter as enqueue_denoise / enqueue_variance run it with out = nullptr, or launch_denoise_prep alone; then the
// kernel, from the float image and the compact guide and keys in the context's scratch, into `out`.
hrt_status enqueue_upsample(hrt_context* ctx, const hrt_upsample_info* info, const hrt_denoise_info* denoise,
                            const hrt_variance_info* variance, const hrt_hit* low_hits, const hrt_hit* high_hits, void* out,
                            int out_kind, uint32_t pitch, uint32_t bgra, const char* who) {
  hrt_status st;
  void* low = nullptr;
  if (denoise) {
    if ((st = enqueue_denoise(ctx, denoise, low_hits, nullptr, false, &low, who)) != HRT_OK) return st;
  } else if (variance) {
    if ((st = enqueue_variance(ctx, variance, low_hits, nullptr, false, nullptr, &low, who)) != HRT_OK) return st;
  } else {
    const size_t np = ctx->npix();
    if ((st = ensure_staging(ctx, &ctx->dn_img[0], np * 16, who)) != HRT_OK) return st;
    if ((st = ensure_staging(ctx, &ctx->dn_guide, np * 16, who)) != HRT_OK) return st;
    if ((st = ensure_staging(ctx, &ctx->dn_keys, np * 4, who)) != HRT_OK) return st;
    const void* src = hrt::local_image(ctx, info->image_id);
    if (!src) return fail(ctx, HRT_ERR_HIP, std::string(who) + ": lane wait failed");
    HRT_HIP(ctx, hrt::launch_denoise_prep(src, ctx->f32(), low_hits, ctx->dn_img[0], ctx->dn_guide, ctx->dn_keys, np, ctx->stream));
    if (info->image_id == HRT_IMG_TRACE) {
      // prep was the source's only reader: the trace image's next writer follows it (enqueue_denoise's rule)
      if (ctx->cur_slot >= 0) {
        HRT_HIP(ctx, hipEventRecord(ctx->fold_done, ctx->stream));
        ctx->fold_set = true;
      }
      if ((st = hrt::release_lane(ctx, ctx->cur_lane)) != HRT_OK) return st;
    }
    low = ctx->dn_img[0];
  }
  // S19's host constant, one rounded float operation
  const hrt::UpsamplePass p{low, ctx->dn_guide, ctx->dn_keys, high_hits, out, out_kind, ctx->width, ctx->local_rows,
                            info->width, info->height, pitch, bgra, info->footprint, 1.0f / info->sigma_normal,
                            info->sigma_depth};
  HRT_HIP(ctx, hrt::launch_upsample(p, ctx->stream));
  return HRT_OK;
}

}  // namespace

extern "C" void hrt_upsample_defaults(hrt_upsample_info* info, uint32_t width, uint32_t height) {
  if (!info) return;
  *info = hrt_upsample_info{HRT_IMG_ACCUM, width, height, HRT_UPSAMPLE_FOOTPRINT, 0u, HRT_DENOISE_SIGMA_NORMAL,
                            HRT_DENOISE_SIGMA_DEPTH, 0u};
}

extern "C" hrt_status hrt_upsample(hrt_context* ctx, const hrt_upsample_info* info, const hrt_denoise_info* denoise,
                                   const hrt_variance_info* variance, const hrt_hit* low_hits, const hrt_hit* high_hits,
                                   uint32_t fmt, void* dst, size_t bytes) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_upsample";
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  hrt_status st = check_upsample(ctx, info, denoise, variance, low_hits, high_hits, who);
  if (st != HRT_OK) return st;
  if (fmt != HRT_FMT_RGBA8 && fmt != HRT_FMT_RGBA32F) return bad("unknown format");
  if (!dst) return bad("null destination");
  const bool rgba8 = fmt == HRT_FMT_RGBA8;
  const size_t need = (size_t)info->width * info->height * (rgba8 ? 4 : 16);
  if (bytes < need) return bad("destination too small");
  // device memory a texel store may address: the kernel writes it; anything else is copied from the staging image
  const bool direct = (uintptr_t)dst % (rgba8 ? 4 : 16) == 0 && query_direct(ctx, dst) &&
                      query_direct(ctx, static_cast<const char*>(dst) + (need - 1));
  void* out = dst;
  if (!direct) {
    if (ctx->up_stage && ctx->up_stage_bytes < need) {  // (the call is blocking: no earlier result is in flight)
      free_dev(ctx, ctx->up_stage);
      ctx->up_stage_bytes = 0;
    }
    if ((st = ensure_staging(ctx, &ctx->up_stage, need, who)) != HRT_OK) return st;
    if (ctx->up_stage_bytes < need) ctx->up_stage_bytes = need;
    out = ctx->up_stage;
  }
  if ((st = enqueue_upsample(ctx, info, denoise, variance, low_hits, high_hits, out,
                             rgba8 ? hrt::kUpsampleOutRgba8 : hrt::kUpsampleOutFloat, 0u, 0u, who)) != HRT_OK)
    return st;
  if (!direct) HRT_HIP(ctx, hipMemcpyAsync(dst, out, need, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HRT_OK;
}

extern "C" hrt_status hrt_upsample_present(hrt_context* ctx, const hrt_upsample_info* info, const hrt_denoise_info* denoise,
                                           const hrt_variance_info* variance, const hrt_hit* low_hits,
                                           const hrt_hit* high_hits, const hrt_present_info* target, void* dst,
                                           uint64_t dst_bytes, uint64_t* ticket) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_upsample_present";
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  hrt_status st = check_upsample(ctx, info, denoise, variance, low_hits, high_hits, who);
  if (st != HRT_OK) return st;
  if ((st = check_present(ctx, target, dst, dst_bytes, ticket, false, who)) != HRT_OK) return st;
  if (target->image_id != info->image_id) return bad("the target's image_id differs from info's");
  if (target->width != info->width || target->height != info->height) return bad("the target's size differs from info's");
  hipEvent_t ev = nullptr;
  if ((st = ticket_begin(ctx, &ev)) != HRT_OK) return st;
  // the kernel writes the flipped, swizzled target pixel: the result is never written to memory and read back
  if ((st = enqueue_upsample(ctx, info, denoise, variance, low_hits, high_hits, dst, hrt::kUpsampleOutPresent, target->pitch,
                             target->format == HRT_PRESENT_B8G8R8A8 ? 1u : 0u, who)) != HRT_OK)
    return st;
  return ticket_end(ctx, ev, ticket);
}

extern "C" hrt_status hrt_order_after(hrt_context* ctx, hrt_context* producer) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  if (!producer) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_order_after: null producer");
  if (ctx == producer) return HRT_OK;
  if (ctx->device != producer->device)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_order_after: the two contexts are on different devices");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if (!producer->order_ev) HRT_HIP(ctx, hipEventCreateWithFlags(&producer->order_ev, hipEventDisableTiming));
  HRT_HIP(ctx, hipEventRecord(producer->order_ev, producer->stream));
  HRT_HIP(ctx, hipStreamWaitEvent(ctx->stream, producer->order_ev, 0));
  return HRT_OK;
}

// ---- temporal upsampling (kernel in hrt_resolve.hip) -------------------------------------
extern "C" void hrt_resolve_defaults(hrt_resolve_info* info) {
  if (!info) return;
  *info = hrt_resolve_info{0.0f, 0.0f, 32u, HRT_RESOLVE_FILL, {0u, 0u, 0u, 0u}};
}

extern "C" void hrt_history_phase(uint32_t ws, uint32_t w, uint32_t hs, uint32_t h, uint32_t k, float* ox, float* oy) {
  const uint32_t nx = hrt::resolve_phases(ws, w), ny = hrt::resolve_phases(hs, h);
  if (ox) *ox = hrt::resolve_phase_offset(k % nx, nx);
  if (oy) *oy = hrt::resolve_phase_offset((k / nx) % ny, ny);
}

// The ray centres are read by the traces on the lane streams and by everything else on the context's stream: the
// write runs on the context's stream after every lane's latest trace (join_lanes), and every lane's next trace
// waits for it through the lane's `free` event, as it waits for the last reader of its buffers.
extern "C" hrt_status hrt_set_ray_grid(hrt_context* ctx, const float first[3], const float dx[3], const float dy[3]) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string("hrt_set_ray_grid: ") + what); };
  if (!first || !dx || !dy) return bad("null first, dx or dy");
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(first[c]) || !std::isfinite(dx[c]) || !std::isfinite(dy[c])) return bad("a component is not finite");
  if (ctx->comm || ctx->part_count > 1)
    return bad("a context of a row-tile partition or joined to a communicator takes its rays from hrt_set_scene or "
               "hrt_generate_rays (the stream-ordered passes that need a shifted grid refuse such a context)");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  const size_t want = (size_t)ctx->width * ctx->height;
  if (!ctx->scene.rays || ctx->n_rays != want) {  // (no buffer of this size: nothing in flight reads one)
    free_dev(ctx, ctx->scene.rays);
    ctx->n_rays = 0;
    HRT_HIP(ctx, hrt::dev_alloc(ctx, (void**)&ctx->scene.rays, (want ? want : 1) * sizeof(float4)));
  }
  if ((st = hrt::join_lanes(ctx)) != HRT_OK) return st;
  for (auto& l : ctx->lane) l.tl_ready = false;  // the tile lists were built from the old ray centres
  HRT_HIP(ctx, hrt::launch_make_rays(ctx->scene.rays, ctx->width, ctx->height, first, dx, dy, ctx->stream));
  ctx->n_rays = (uint32_t)want;
  for (int l = 0; l < hrt::kLanes; ++l)
    if ((st = hrt::release_lane(ctx, l)) != HRT_OK) return st;
  return HRT_OK;
}

extern "C" hrt_status hrt_accumulate_history_from(hrt_context* ctx, hrt_context* source, const hrt_resolve_info* info,
                                                  const hrt_hit* source_hits, const hrt_hit* hits) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_accumulate_history_from";
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  if (!source) return bad("null source");
  if (!info) return bad("null info");
  if (ctx->device != source->device) return bad("the two contexts are on different devices");
  if (ctx->mode != source->mode) return bad("the two contexts are in different modes");
  if (!(std::isfinite(info->offset_x) && std::isfinite(info->offset_y) && info->offset_x >= -0.5f && info->offset_x <= 0.5f &&
        info->offset_y >= -0.5f && info->offset_y <= 0.5f))
    return bad("the offsets must be finite and in [-0.5, 0.5]");
  if (info->max_history == 0 || info->max_history > hrt::kHistoryMax) return bad("max_history must be 1..2^24");
  if (info->flags & ~(HRT_RESOLVE_FILL | HRT_RESOLVE_MOMENTS)) return bad("unknown flag bits");
  if ((source_hits == nullptr) != (hits == nullptr)) return bad("source_hits and hits must both be given or both be NULL");
  if (ctx->comm || ctx->part_count > 1) return begin_history(ctx, who);  // (the rejection)
  if (source->comm || source->part_count > 1)
    return bad("the source is a context of a row-tile partition or joined to a communicator (its trace image is not a frame)");
  if (source != ctx && !source->scene_set) return fail(ctx, HRT_ERR_NO_SCENE, std::string(who) + ": the source has no scene (no trace image to fold)");
  if (ctx->width > (1u << 24) || ctx->height > (1u << 24) || source->width > (1u << 24) || source->height > (1u << 24))
    return bad("an image is wider or taller than 2^24");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if (hits) {
    if ((uintptr_t)source_hits % 16 != 0 || (uintptr_t)hits % 16 != 0) return bad("source_hits and hits must be 16-byte aligned");
    if (!hits_on_device(source, source_hits))
      return bad("source_hits must be the source's width x height records in memory of the contexts' device");
    if (!hits_on_device(ctx, hits)) return bad("hits must be width x height records in memory of the contexts' device");
  }
  const bool moments = (info->flags & HRT_RESOLVE_MOMENTS) != 0;
  if ((st = begin_history(ctx, who)) != HRT_OK) return st;
  if (moments && (st = begin_moments(ctx, who)) != HRT_OK) return st;
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;  // frames fold in call order
  // T: after the source's deferred combines and its latest trace, as accumulate_history_call orders them on the
  // source's stream; then this stream follows the source's
  const int l = source->cur_lane;
  if (source != ctx) {
    if ((st = hrt::flush_combines(source)) != HRT_OK) return fail(ctx, st, std::string(who) + ": " + source->err);
    if ((st = hrt::wait_lane(source, l)) != HRT_OK) return fail(ctx, st, std::string(who) + ": " + source->err);
    if (!source->order_ev) HRT_HIP(ctx, hipEventCreateWithFlags(&source->order_ev, hipEventDisableTiming));
    HRT_HIP(ctx, hipEventRecord(source->order_ev, source->stream));
    HRT_HIP(ctx, hipStreamWaitEvent(ctx->stream, source->order_ev, 0));
  } else if ((st = hrt::wait_lane(ctx, l)) != HRT_OK) {
    return st;
  }
  const hrt::ResolvePass pass{ctx->accum, ctx->hist_cnt, moments ? ctx->hist_mom : nullptr, hrt::trace_image(source),
                              source_hits, hits, ctx->f32(), source->width, source->local_rows, ctx->width, ctx->local_rows,
                              info->offset_x, info->offset_y, info->max_history, info->flags & HRT_RESOLVE_FILL};
  HRT_HIP(ctx, hrt::launch_resolve(pass, ctx->stream));
  ctx->accumulates++;
  // T's next writer -- the source's next trace into this lane or ring slot -- waits for the kernel
  if (source == ctx) {  // accumulate_history_call's own steps
    if (ctx->cur_slot >= 0) {
      HRT_HIP(ctx, hipEventRecord(ctx->fold_done, ctx->stream));
      ctx->fold_set = true;
    }
    return hrt::release_lane(ctx, l);
  }
  // A reader on another stream: the source's `free` and `fold_done` cannot carry it, because the source's own
  // calls (hrt_set_ray_grid, hrt_accumulate, a read of the trace image, a flush of its combines) re-record them
  // on its own stream, which does not wait for this one, and the newer record would hide this reader.  So the
  // lane and the ring have an event of their own for such readers, recorded only here, and every writer of the
  // image waits for both.  An earlier record of it (another target's fold) is waited for first, so that the one
  // event stands for every foreign reader so far.
  hrt::Lane& sl = source->lane[l];
  if (!sl.foreign) HRT_HIP(ctx, hipEventCreateWithFlags(&sl.foreign, hipEventDisableTiming));
  if (sl.foreign_set) HRT_HIP(ctx, hipStreamWaitEvent(ctx->stream, sl.foreign, 0));
  HRT_HIP(ctx, hipEventRecord(sl.foreign, ctx->stream));
  sl.foreign_set = true;
  if (source->cur_slot >= 0) {
    if (!source->fold_foreign) HRT_HIP(ctx, hipEventCreateWithFlags(&source->fold_foreign, hipEventDisableTiming));
    if (source->fold_foreign_set) HRT_HIP(ctx, hipStreamWaitEvent(ctx->stream, source->fold_foreign, 0));
    HRT_HIP(ctx, hipEventRecord(source->fold_foreign, ctx->stream));
    source->fold_foreign_set = true;
  }
  return HRT_OK;
}

// ---- adaptive refinement (kernels in hrt_refine.hip) ------------------------------------
namespace {

// AUTO: FRAME.  At 1080p, 64 spp (profiles/refine_rate.jsonl) a FRAME pass costs the frame whatever the
// share -- island 2.9 to 3.2 ms, cave 10.2 to 10.6 -- and a QUERIES pass starts at the latency of one lane's 64 samples
// (island 5.7 ms at 1 % of the pixels, cave 8.4) and grows with the share: on island FRAME wins at every share
// measured with the ranges apart, on cave from 10 % on, with the ranges overlapping at 5 % and QUERIES ahead at 1 %
// (8.4 against 10.3).  No threshold on the share serves both scenes, so AUTO does not look at it.
constexpr uint32_t kRefineAuto = HRT_REFINE_FRAME;

hrt_status check_refine_rule(hrt_context* ctx, const hrt_refine_rule* rule, const char* who) {
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  if (!rule) return bad("null rule");
  if (rule->flags != 0) return bad("rule flags must be 0");
  if (rule->min_history == 0) return bad("min_history must be at least 1");
  if (rule->max_count < rule->min_history) return bad("max_count must be at least min_history");
  if (rule->radius > HRT_REFINE_MAX_RADIUS) return bad("radius must be 0..3");
  if (!(std::isfinite(rule->tolerance) && rule->tolerance > 0.0f)) return bad("tolerance must be finite and > 0");
  if (!(std::isfinite(rule->luminance_floor) && rule->luminance_floor > 0.0f))
    return bad("luminance_floor must be finite and > 0");
  return HRT_OK;
}

// The guide of a selection: NULL, or width x height records of the context's device, 16-byte aligned.
hrt_status check_refine_guide(hrt_context* ctx, const hrt_hit* guide, const char* who) {
  if (!guide) return HRT_OK;
  if ((uintptr_t)guide % 16 != 0)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": the guide must be 16-byte aligned");
  if (!hits_on_device(ctx, guide))
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT,
                std::string(who) + ": the guide must be width x height records in memory of the context's device");
  return HRT_OK;
}

// What hrt_refine checks of its own arguments (hrt_refine_until too, before its first pass).
hrt_status check_refine(hrt_context* ctx, const hrt_push_constants* pc, uint32_t max_history, uint32_t method,
                        uint32_t query_method, uint32_t flags, const char* who) {
  auto bad = [&](const char* what) { return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
  if (!pc) return bad("null push block");
  if (method > HRT_REFINE_FRAME) return bad("unknown method");
  if (!known_query_method(query_method)) return bad("unknown query method");
  if (flags & ~HRT_REFINE_MOMENTS) return bad("flag bits other than HRT_REFINE_MOMENTS");
  if (max_history == 0 || max_history > hrt::kHistoryMax) return bad("max_history must be 1..2^24");
  if (pc->init) return bad("pc->init must be 0");
  if (ctx->comm || ctx->part_count > 1) return begin_history(ctx, who);  // (the rejection)
  return check_dispatch(ctx, pc, who);
}

size_t refine_mask_words(const hrt_context* ctx) { return (ctx->npix() + 31) / 32; }

// The context's staging mask and its two words.
hrt_status ensure_refine_words(hrt_context* ctx, const char* who) {
  void* p = ctx->rf_words;
  hrt_status st = ensure_staging(ctx, &p, 2 * sizeof(unsigned long long), who);
  ctx->rf_words = static_cast<unsigned long long*>(p);
  return st;
}
hrt_status ensure_refine_mask(hrt_context* ctx, const char* who) {
  void* p = ctx->rf_mask;
  hrt_status st = ensure_staging(ctx, &p, refine_mask_words(ctx) * 4, who);
  ctx->rf_mask = static_cast<uint32_t*>(p);
  return st;
}

// The selection into dmask (device memory), enqueued on ctx->stream; the count lands in rf_words[0].  Every
// argument has been checked.
hrt_status enqueue_refine_select(hrt_context* ctx, const hrt_refine_rule* rule, const hrt_hit* guide, uint32_t* dmask,
                                 const char* who) {
  hrt_status st = begin_history(ctx, who);
  if (st != HRT_OK) return st;
  if ((st = begin_moments(ctx, who)) != HRT_OK) return st;
  if ((st = ensure_refine_words(ctx, who)) != HRT_OK) return st;
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;
  HRT_HIP(ctx, hipMemsetAsync(ctx->rf_words, 0, sizeof(unsigned long long), ctx->stream));
  const hrt::RefineRuleK k{rule->min_history, rule->max_count, rule->radius, rule->tolerance * rule->tolerance,
                           rule->luminance_floor};
  HRT_HIP(ctx, hrt::launch_refine_select(ctx->hist_cnt, ctx->hist_mom, guide, dmask, ctx->rf_words, ctx->width,
                                         ctx->local_rows, k, ctx->stream));
  return HRT_OK;
}

// One refinement pass over dmask (device memory).  Every argument has been checked.
hrt_status refine_pass(hrt_context* ctx, const hrt_push_constants* pc, const uint32_t* dmask, uint32_t max_history,
                       uint32_t method, uint32_t query_method, uint32_t flags, hrt_refine_stats* stats, const char* who) {
  const bool moments = (flags & HRT_REFINE_MOMENTS) != 0;
  const uint32_t np = (uint32_t)ctx->npix();
  const uint32_t ran = method == HRT_REFINE_AUTO ? kRefineAuto : method;
  hrt_status st = begin_history(ctx, who);
  if (st != HRT_OK) return st;
  if (moments && (st = begin_moments(ctx, who)) != HRT_OK) return st;
  if ((st = ensure_refine_words(ctx, who)) != HRT_OK) return st;
  if (ran == HRT_REFINE_QUERIES) {
    if ((st = ensure_staging(ctx, &ctx->rf_queries, (size_t)np * sizeof(hrt_radiance_query), who)) != HRT_OK) return st;
    void* p = ctx->rf_index;
    if ((st = ensure_staging(ctx, &p, (size_t)np * 4, who)) != HRT_OK) return st;
    ctx->rf_index = static_cast<uint32_t*>(p);
    if ((st = ensure_staging(ctx, &ctx->rf_rgba, (size_t)np * 16, who)) != HRT_OK) return st;
    if ((st = ensure_staging(ctx, reinterpret_cast<void**>(&ctx->rad_words), 4 * sizeof(unsigned long long), who)) != HRT_OK)
      return st;
  }
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;
  // the list (QUERIES) or the count alone (FRAME), and the count back to the host
  uint32_t* next = reinterpret_cast<uint32_t*>(ctx->rf_words + 1);
  HRT_HIP(ctx, hipMemsetAsync(next, 0, sizeof(unsigned long long), ctx->stream));
  const bool list = ran == HRT_REFINE_QUERIES;
  HRT_HIP(ctx, hrt::launch_refine_queries(dmask, ctx->scene.rays, list ? static_cast<float4*>(ctx->rf_queries) : nullptr,
                                          ctx->rf_index, next, np, pc->cam_pos, pc->rng_offset * 719393u, ctx->stream));
  uint32_t n = 0;
  HRT_HIP(ctx, hipMemcpyAsync(&n, next, sizeof n, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) *stats = hrt_refine_stats{0u, 0u, n, 0u, 0u, 0u, 0u};
  if (n == 0) return HRT_OK;
  float* mom = moments ? ctx->hist_mom : nullptr;
  if (list) {
    hrt::TraceParams p = make_params(ctx, pc, 0);
    const hrt::QueryPlan plan =
        hrt::plan_query(hrt::plan_scene(p), query_method == HRT_QUERY_AUTO ? (int)HRT_QUERY_PAIRS : (int)query_method);
    query_only(p);
    if (stats) HRT_HIP(ctx, hipMemsetAsync(ctx->rad_words, 0, 3 * sizeof(unsigned long long), ctx->stream));
    for (uint32_t at = 0; at < n; at += std::min(kQueryLaunch, n - at)) {
      hrt::RadianceArgs q{};
      q.queries = static_cast<const float4*>(ctx->rf_queries) + 2 * (size_t)at;
      q.out = static_cast<float4*>(ctx->rf_rgba) + at;
      q.stats = stats ? ctx->rad_words : nullptr;
      q.next = reinterpret_cast<uint32_t*>(ctx->rad_words + 3);
      q.n = std::min(kQueryLaunch, n - at);
      HRT_HIP(ctx, hrt::launch_radiance(p, q, plan, ctx->stream));
    }
    HRT_HIP(ctx, hrt::launch_refine_fold(ctx->accum, ctx->hist_cnt, mom, ctx->f32(), static_cast<const float4*>(ctx->rf_rgba),
                                         ctx->rf_index, n, max_history, ctx->stream));
    unsigned long long counts[3] = {0, 0, 0};
    if (stats) HRT_HIP(ctx, hipMemcpyAsync(counts, ctx->rad_words, sizeof(counts), hipMemcpyDefault, ctx->stream));
    HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) *stats = hrt_refine_stats{ran, (uint32_t)plan.method, n, counts[0], counts[1], counts[2], 0u};
    return HRT_OK;
  }
  // FRAME: the frame kernel, then fold_history's lane protocol around the masked fold
  if ((st = hrt_trace(ctx, pc)) != HRT_OK) return st;
  const int l = ctx->cur_lane;
  if ((st = hrt::wait_lane(ctx, l)) != HRT_OK) return st;
  HRT_HIP(ctx, hrt::launch_refine_fold_image(ctx->accum, hrt::trace_image(ctx), ctx->hist_cnt, mom, ctx->f32(), dmask, np,
                                             max_history, ctx->stream));
  if (ctx->cur_slot >= 0) {  // a slot of the deferred combiner's ring: its next trace waits for this fold
    HRT_HIP(ctx, hipEventRecord(ctx->fold_done, ctx->stream));
    ctx->fold_set = true;
  }
  if ((st = hrt::release_lane(ctx, l)) != HRT_OK) return st;
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) stats->method_ran = ran;
  return HRT_OK;
}

}  // namespace

extern "C" void hrt_refine_defaults(hrt_refine_rule* rule) {
  if (!rule) return;
  *rule = hrt_refine_rule{HRT_REFINE_MIN_HISTORY, HRT_REFINE_MAX_COUNT, HRT_REFINE_RADIUS, 0u,
                          HRT_REFINE_TOLERANCE,   HRT_REFINE_FLOOR,     {0u, 0u}};
}

extern "C" hrt_status hrt_refine_select(hrt_context* ctx, const hrt_refine_rule* rule, const hrt_hit* guide, uint32_t* mask,
                                        uint64_t* selected) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_refine_select";
  hrt_status st = check_refine_rule(ctx, rule, who);
  if (st != HRT_OK) return st;
  if (!mask) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_refine_select: null mask");
  if (ctx->comm || ctx->part_count > 1) return begin_history(ctx, who);  // (the rejection)
  if ((st = bind(ctx)) != HRT_OK) return st;
  if ((st = check_refine_guide(ctx, guide, who)) != HRT_OK) return st;
  const size_t words = refine_mask_words(ctx);
  const bool direct = query_direct(ctx, mask);
  if (direct && (uintptr_t)mask % 4 != 0)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_refine_select: a device mask must be 4-byte aligned");
  if (!direct && (st = ensure_refine_mask(ctx, who)) != HRT_OK) return st;
  if ((st = enqueue_refine_select(ctx, rule, guide, direct ? mask : ctx->rf_mask, who)) != HRT_OK) return st;
  if (direct && !selected) return HRT_OK;
  if (!direct) HRT_HIP(ctx, hipMemcpyAsync(mask, ctx->rf_mask, words * 4, hipMemcpyDefault, ctx->stream));
  unsigned long long count = 0;
  HRT_HIP(ctx, hipMemcpyAsync(&count, ctx->rf_words, sizeof count, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (selected) *selected = count;
  return HRT_OK;
}

extern "C" hrt_status hrt_refine(hrt_context* ctx, const hrt_push_constants* pc, const uint32_t* mask, uint32_t max_history,
                                 uint32_t method, uint32_t query_method, uint32_t flags, hrt_refine_stats* stats) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_refine";
  hrt_status st = check_refine(ctx, pc, max_history, method, query_method, flags, who);
  if (st != HRT_OK) return st;
  if (!mask) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_refine: null mask");
  if ((st = bind(ctx)) != HRT_OK) return st;
  const bool direct = query_direct(ctx, mask);
  if (direct && (uintptr_t)mask % 4 != 0)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_refine: a device mask must be 4-byte aligned");
  if (!direct) {
    if ((st = ensure_refine_mask(ctx, who)) != HRT_OK) return st;
    HRT_HIP(ctx, hipMemcpyAsync(ctx->rf_mask, mask, refine_mask_words(ctx) * 4, hipMemcpyDefault, ctx->stream));
  }
  return refine_pass(ctx, pc, direct ? mask : ctx->rf_mask, max_history, method, query_method, flags, stats, who);
}

extern "C" hrt_status hrt_refine_until(hrt_context* ctx, const hrt_push_constants* pc, const hrt_refine_rule* rule,
                                       const hrt_hit* guide, uint32_t max_history, uint32_t max_passes, uint32_t method,
                                       uint32_t flags, uint32_t* passes_done, uint64_t* pixel_frames, uint32_t* settled) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_refine_until";
  if (!passes_done || !pixel_frames)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_refine_until: null passes_done or pixel_frames");
  hrt_status st = check_refine_rule(ctx, rule, who);
  if (st != HRT_OK) return st;
  if ((st = check_refine(ctx, pc, max_history, method, HRT_QUERY_AUTO, flags, who)) != HRT_OK) return st;
  if ((st = bind(ctx)) != HRT_OK) return st;
  if ((st = check_refine_guide(ctx, guide, who)) != HRT_OK) return st;
  if ((st = ensure_refine_mask(ctx, who)) != HRT_OK) return st;
  *passes_done = 0;
  *pixel_frames = 0;
  if (settled) *settled = 0;
  hrt_push_constants frame = *pc;
  for (uint32_t k = 0; k < max_passes; ++k) {
    if ((st = enqueue_refine_select(ctx, rule, guide, ctx->rf_mask, who)) != HRT_OK) return st;
    unsigned long long count = 0;
    HRT_HIP(ctx, hipMemcpyAsync(&count, ctx->rf_words, sizeof count, hipMemcpyDefault, ctx->stream));
    HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (count == 0) {
      if (settled) *settled = 1;
      break;
    }
    frame.rng_offset = pc->rng_offset + k;
    if ((st = refine_pass(ctx, &frame, ctx->rf_mask, max_history, method, HRT_QUERY_AUTO, flags | HRT_REFINE_MOMENTS, nullptr,
                          who)) != HRT_OK)
      return st;
    *passes_done = k + 1;
    *pixel_frames += count;
  }
  return HRT_OK;
}

// ---- tile-masked refinement (kernels in hrt_refine.hip) ----------------------------------
namespace {

constexpr uint32_t kMaskedTilesMax = (1u << 22) - 1u;  // the item word's tile field (hrt_plan.h kItemTileMask)

// The pass's buffers: the tile bitmap and its counts, and -- plan -- the masked launches' own sched, items and costs.
hrt_status ensure_refine_tiles(hrt_context* ctx, bool plan, const char* who) {
  const size_t tiles = ctx->num_tiles();
  auto ensure = [&](auto*& field, size_t bytes) {
    void* p = field;
    hrt_status st = ensure_staging(ctx, &p, bytes, who);
    field = static_cast<std::remove_reference_t<decltype(field)>>(p);
    return st;
  };
  hrt_status st = ensure(ctx->rt_bits, (tiles + 31) / 32 * 4);
  if (st == HRT_OK) st = ensure(ctx->rt_counts, 3 * sizeof(unsigned long long));
  if (plan && st == HRT_OK) st = ensure(ctx->rt_sched, hrt::kSchedWords * 4);
  if (plan && st == HRT_OK) st = ensure(ctx->rt_items, tiles * 64 * 4);
  if (plan && st == HRT_OK) st = ensure(ctx->rt_cost, tiles * 4);
  return st;
}

// What hrt_refine_tiles checks beyond check_refine.
hrt_status check_refine_tiles(hrt_context* ctx, const hrt_push_constants* pc, uint32_t max_history, uint32_t frames,
                              uint32_t flags, const char* who) {
  hrt_status st = check_refine(ctx, pc, max_history, HRT_REFINE_FRAME, HRT_QUERY_AUTO, flags, who);
  if (st != HRT_OK) return st;
  if (frames == 0 || frames > HRT_REFINE_TILES_MAX_FRAMES)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, std::string(who) + ": frames must be 1..HRT_REFINE_TILES_MAX_FRAMES");
  return HRT_OK;
}

// One tile-masked pass of `frames` frames over dmask (device memory).  Every argument has been checked.
hrt_status refine_tiles_pass(hrt_context* ctx, const hrt_push_constants* pc, const uint32_t* dmask, uint32_t max_history,
                             uint32_t frames, uint32_t flags, hrt_refine_tiles_stats* stats, const char* who) {
  const bool moments = (flags & HRT_REFINE_MOMENTS) != 0;
  hrt_status st = begin_history(ctx, who);
  if (st != HRT_OK) return st;
  if (moments && (st = begin_moments(ctx, who)) != HRT_OK) return st;
  // host side: the kernel the request resolves to decides between the masked launches and whole frames
  const hrt::TraceParams p0 = make_params(ctx, pc, 0);
  const hrt::LaunchPlan plan = hrt::plan_trace(hrt::plan_scene(p0), ctx->variant);
  const uint32_t tiles = (uint32_t)ctx->num_tiles();
  const bool whole = !hrt::kernel_traits(plan.kernel).persistent || ctx->num_tiles() > kMaskedTilesMax || ctx->diag_on;
  if ((st = ensure_refine_tiles(ctx, !whole, who)) != HRT_OK) return st;
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;
  // the tile bitmap and the counts, back to the host
  HRT_HIP(ctx, hipMemsetAsync(ctx->rt_counts, 0, 3 * sizeof(unsigned long long), ctx->stream));
  HRT_HIP(ctx, hrt::launch_refine_tile_bits(dmask, ctx->rt_bits, ctx->rt_counts, ctx->width, ctx->local_rows, ctx->stream));
  unsigned long long counts[3] = {0, 0, 0};
  HRT_HIP(ctx, hipMemcpyAsync(counts, ctx->rt_counts, sizeof counts, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) *stats = hrt_refine_tiles_stats{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (counts[0] == 0) return HRT_OK;
  Batch b;
  if ((st = begin_batch(ctx, pc, frames, UINT32_MAX, &b)) != HRT_OK) return st;
  hrt::Lane& lane = ctx->lane[0];
  const hrt::MaskedPlan mp{ctx->rt_bits, ctx->rt_sched, ctx->rt_items, ctx->rt_cost, (uint32_t)counts[1], lane.plan_valid};
  float* mom = moments ? ctx->hist_mom : nullptr;
  for (uint32_t done = 0; done < frames;) {
    // hrt_compute_n's near-equal launches
    const uint32_t left = frames - done, launches = (left + b.lcap - 1) / b.lcap;
    const uint32_t nf = (left + launches - 1) / launches, frame0 = pc->rng_offset + done;
    const char* stack = nullptr;
    if ((st = launch_batch(ctx, b, frame0, nf, &stack, whole ? nullptr : &mp)) != HRT_OK) return st;
    // the fold under the mask; a masked launch's last frame goes to lane 0's image tile by tile, a whole one's whole
    void* trace = !whole && nf > 1 ? lane.trace : nullptr;
    HRT_HIP(ctx, hrt::launch_refine_fold_frames(ctx->accum, stack, ctx->npix(), nf, ctx->hist_cnt, mom, ctx->f32(), dmask,
                                                trace ? ctx->rt_bits : nullptr, trace, ctx->width, ctx->local_rows,
                                                max_history, ctx->stream));
    if (whole && (st = keep_last_frame(ctx, stack, nf, nf)) != HRT_OK) return st;
    done += nf;
  }
  if ((st = end_batch(ctx)) != HRT_OK) return st;
  uint32_t items = 0;
  if (!whole && stats) HRT_HIP(ctx, hipMemcpyAsync(&items, ctx->rt_sched + 1, sizeof items, hipMemcpyDefault, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats)
    *stats = hrt_refine_tiles_stats{(uint32_t)plan.kernel, whole ? 1u : 0u, tiles, (uint32_t)counts[1], items, 0u, counts[0],
                                    whole ? (uint64_t)ctx->npix() : counts[2]};
  return HRT_OK;
}

}  // namespace

extern "C" hrt_status hrt_refine_tiles(hrt_context* ctx, const hrt_push_constants* pc, const uint32_t* mask, uint32_t max_history,
                                       uint32_t frames, uint32_t flags, hrt_refine_tiles_stats* stats) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_refine_tiles";
  hrt_status st = check_refine_tiles(ctx, pc, max_history, frames, flags, who);
  if (st != HRT_OK) return st;
  if (!mask) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_refine_tiles: null mask");
  if ((st = bind(ctx)) != HRT_OK) return st;
  const bool direct = query_direct(ctx, mask);
  if (direct && (uintptr_t)mask % 4 != 0)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_refine_tiles: a device mask must be 4-byte aligned");
  if (!direct) {
    if ((st = ensure_refine_mask(ctx, who)) != HRT_OK) return st;
    HRT_HIP(ctx, hipMemcpyAsync(ctx->rf_mask, mask, refine_mask_words(ctx) * 4, hipMemcpyDefault, ctx->stream));
  }
  return refine_tiles_pass(ctx, pc, direct ? mask : ctx->rf_mask, max_history, frames, flags, stats, who);
}

extern "C" hrt_status hrt_refine_tiles_until(hrt_context* ctx, const hrt_push_constants* pc, const hrt_refine_rule* rule,
                                             const hrt_hit* guide, uint32_t max_history, uint32_t max_passes,
                                             uint32_t frames_per_pass, uint32_t flags, uint32_t* passes_done,
                                             uint64_t* pixel_frames, uint32_t* settled) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  const char* who = "hrt_refine_tiles_until";
  if (!passes_done || !pixel_frames)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_refine_tiles_until: null passes_done or pixel_frames");
  hrt_status st = check_refine_rule(ctx, rule, who);
  if (st != HRT_OK) return st;
  if ((st = check_refine_tiles(ctx, pc, max_history, frames_per_pass, flags, who)) != HRT_OK) return st;
  if ((st = bind(ctx)) != HRT_OK) return st;
  if ((st = check_refine_guide(ctx, guide, who)) != HRT_OK) return st;
  if ((st = ensure_refine_mask(ctx, who)) != HRT_OK) return st;
  *passes_done = 0;
  *pixel_frames = 0;
  if (settled) *settled = 0;
  hrt_push_constants frame = *pc;
  for (uint32_t k = 0; k < max_passes; ++k) {
    if ((st = enqueue_refine_select(ctx, rule, guide, ctx->rf_mask, who)) != HRT_OK) return st;
    unsigned long long count = 0;
    HRT_HIP(ctx, hipMemcpyAsync(&count, ctx->rf_words, sizeof count, hipMemcpyDefault, ctx->stream));
    HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (count == 0) {
      if (settled) *settled = 1;
      break;
    }
    frame.rng_offset = pc->rng_offset + k * frames_per_pass;
    if ((st = refine_tiles_pass(ctx, &frame, ctx->rf_mask, max_history, frames_per_pass, flags | HRT_REFINE_MOMENTS, nullptr,
                                who)) != HRT_OK)
      return st;
    *passes_done = k + 1;
    *pixel_frames += count * frames_per_pass;
  }
  return HRT_OK;
}

extern "C" hrt_status hrt_present_done(hrt_context* ctx, uint64_t ticket, uint32_t* done) {
  if (!ctx || !done) return HRT_ERR_INVALID_ARGUMENT;
  if (ticket == 0 || ticket > ctx->present_issued)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_present_done: no such ticket");
  *done = 1;  // a ticket older than the ring was waited for when its event was reused
  if (ctx->present_issued - ticket >= hrt_context::kPresentRing) return HRT_OK;
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  const hipError_t e = hipEventQuery(ctx->present_ev[(ticket - 1) % hrt_context::kPresentRing]);
  if (e == hipErrorNotReady)
    *done = 0;
  else if (e != hipSuccess)
    return hip_fail(ctx, e, "hipEventQuery");
  return HRT_OK;
}

extern "C" hrt_status hrt_present_wait(hrt_context* ctx, uint64_t ticket) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  if (ticket == 0 || ticket > ctx->present_issued)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_present_wait: no such ticket");
  if (ctx->present_issued - ticket >= hrt_context::kPresentRing) return HRT_OK;
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  HRT_HIP(ctx, hipEventSynchronize(ctx->present_ev[(ticket - 1) % hrt_context::kPresentRing]));
  return HRT_OK;
}

extern "C" hrt_status hrt_get_layout(const hrt_context* ctx, hrt_layout* out) {
  if (!ctx || !out) return HRT_ERR_INVALID_ARGUMENT;
  out->width = ctx->width;
  out->height = ctx->height;
  out->local_rows = ctx->local_rows;
  out->row_tile = ctx->row_tile;
  out->part_index = ctx->part_index;
  out->part_count = ctx->part_count;
  out->mode = ctx->mode;
  return HRT_OK;
}

extern "C" hrt_status hrt_synchronize(hrt_context* ctx) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if ((st = hrt::flush_combines(ctx)) != HRT_OK) return st;  // every accumulate has run after a sync
  return sync_all(ctx);  // (and every present ticket is done: their events were recorded on ctx->stream)
}

extern "C" hrt_status hrt_get_stats(hrt_context* ctx, hrt_stats* out) {
  if (!ctx || !out) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = hrt_synchronize(ctx);
  if (st != HRT_OK) return st;
  if ((st = harvest_events(ctx)) != HRT_OK) return st;
  unsigned long long c[hrt::kNumCounters] = {};
  HRT_HIP(ctx, hipMemcpy(c, ctx->counters, sizeof c, hipMemcpyDeviceToHost));
  out->segments = c[0];
  out->tri_tests = c[1];
  out->traces = ctx->traces;
  out->accumulates = ctx->accumulates;
  out->wave_steps = c[2];
  out->last_kernel = (uint32_t)ctx->last_kernel;
  out->last_block = (uint32_t)ctx->last_block;
  out->last_frames = ctx->last_frames;
  out->reserved = 0;
  out->last_trace_ms = ctx->last_ms;
  out->total_trace_ms = ctx->total_ms;
  return HRT_OK;
}

extern "C" hrt_status hrt_get_diagnostics(hrt_context* ctx, uint64_t* out, uint32_t count) {
  if (!ctx || !out || count > HRT_NUM_DIAG) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = hrt_synchronize(ctx);
  if (st != HRT_OK) return st;
  unsigned long long c[hrt::kNumCounters] = {};
  HRT_HIP(ctx, hipMemcpy(c, ctx->counters, sizeof c, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < count; ++i) out[i] = c[3 + i];
  return HRT_OK;
}

extern "C" hrt_status hrt_generate_rays(hrt_context* ctx, float camera_focal_length, float viewport_height,
                                        const float up[3], float* default_jitter) {
  if (!ctx || !up) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if ((st = sync_all(ctx)) != HRT_OK) return st;  // no trace in flight reads the rays
  float first[3], px[3], py[3];
  const uint32_t n = hrt_host_ray_grid(ctx->width, ctx->height, camera_focal_length, viewport_height, up, first, px,
                                       py, default_jitter);
  const size_t want = (size_t)ctx->width * ctx->height;
  if (!ctx->scene.rays || ctx->n_rays != want) {
    free_dev(ctx, ctx->scene.rays);
    ctx->n_rays = 0;
    HRT_HIP(ctx, hrt::dev_alloc(ctx, (void**)&ctx->scene.rays, (want ? want : 1) * sizeof(float4)));
  }
  for (auto& l : ctx->lane) l.tl_ready = false;  // the tile lists were built from the old ray centres
  if (n) HRT_HIP(ctx, hrt::launch_make_rays(ctx->scene.rays, ctx->width, ctx->height, first, px, py, ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->n_rays = (uint32_t)want;
  return HRT_OK;
}

extern "C" hrt_status hrt_import_external_memory(hrt_context* ctx, int fd, uint64_t size, uint64_t offset,
                                                 uint64_t bytes, void** dev_ptr) {
  if (!ctx || fd < 0 || !dev_ptr || bytes == 0 || offset + bytes > size)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_import_external_memory: bad fd / size / range");
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  hipExternalMemoryHandleDesc desc{};
  desc.type = hipExternalMemoryHandleTypeOpaqueFd;
  desc.handle.fd = fd;
  desc.size = size;
  hipExternalMemory_t mem = nullptr;
  HRT_HIP(ctx, hipImportExternalMemory(&mem, &desc));
  hipExternalMemoryBufferDesc bd{};
  bd.offset = offset;
  bd.size = bytes;
  void* ptr = nullptr;
  if (hipError_t e = hipExternalMemoryGetMappedBuffer(&ptr, mem, &bd); e != hipSuccess) {
    (void)hipDestroyExternalMemory(mem);
    return hip_fail(ctx, e, "hipExternalMemoryGetMappedBuffer");
  }
  ctx->imports.push_back({mem, ptr, bytes});
  *dev_ptr = ptr;
  return HRT_OK;
}

extern "C" hrt_status hrt_release_external_memory(hrt_context* ctx, void* dev_ptr) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < ctx->imports.size(); ++i) {
    if (ctx->imports[i].ptr == dev_ptr) {
      hrt_status st = hrt_synchronize(ctx);  // no pending write into it
      if (st != HRT_OK) return st;
      HRT_HIP(ctx, hipDestroyExternalMemory(ctx->imports[i].mem));
      ctx->imports.erase(ctx->imports.begin() + (long)i);
      return HRT_OK;
    }
  }
  return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_release_external_memory: not an imported pointer");
}

// Test support: device memory exported as a POSIX fd (HIP virtual memory management), i.e. what the
// presenting API hands to hrt_import_external_memory; *ptr is the exporter's own mapping of it.
extern "C" hrt_status hrt_debug_export_memory(int device, uint64_t bytes, int* fd, void** ptr, uint64_t* size) {
  if (!fd || !ptr || !size || bytes == 0) return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "bad arguments");
  hipError_t e = hipSetDevice(device);
  hipMemAllocationProp prop{};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  prop.requestedHandleTypes = hipMemHandleTypePosixFileDescriptor;
  size_t gran = 0;
  if (e == hipSuccess) e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum);
  const size_t sz = gran ? (bytes + gran - 1) / gran * gran : bytes;
  hipMemGenericAllocationHandle_t h{};
  if (e == hipSuccess) e = hipMemCreate(&h, sz, &prop, 0);
  if (e == hipSuccess) e = hipMemExportToShareableHandle(fd, h, hipMemHandleTypePosixFileDescriptor, 0);
  void* va = nullptr;
  if (e == hipSuccess) e = hipMemAddressReserve(&va, sz, 0, nullptr, 0);
  if (e == hipSuccess) e = hipMemMap(va, sz, 0, h, 0);
  if (e == hipSuccess) {
    hipMemAccessDesc acc{};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    e = hipMemSetAccess(va, sz, &acc, 1);
  }
  if (e == hipSuccess) e = hipMemRelease(h);  // the mapping keeps the allocation alive
  if (e != hipSuccess) {
    g_create_error = std::string("export: ") + hipGetErrorString(e);
    return HRT_ERR_HIP;
  }
  *ptr = va;
  *size = sz;
  return HRT_OK;
}

// Test support: hrt_math.h's shared-reciprocal normalize / division and sqrt paths against the
// compiler's IEEE sequences on n hashed inputs; out = {normalize, div3, sqrt mismatches, fast cases}.
extern "C" hrt_status hrt_debug_math_check(int device, uint32_t n, uint32_t seed, uint64_t out[4]) {
  if (!out) return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_debug_math_check: null out");
  unsigned long long* d = nullptr;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc((void**)&d, 4 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(d, 0, 4 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hrt::launch_math_check(n, seed, d, nullptr);
  if (e == hipSuccess) e = hipMemcpy(out, d, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (d) (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(nullptr, e, "hrt_debug_math_check");
  return HRT_OK;
}

// Test support: the RNG-domain shortcuts (sqrt_rng, spec_sincos_angle) against the general routines
// over all 2^32 u01 states; out = {sqrt mismatches, sincos mismatches}.
extern "C" hrt_status hrt_debug_math_check_rng(int device, uint64_t out[5]) {
  if (!out) return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_debug_math_check_rng: null out");
  unsigned long long* d = nullptr;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc((void**)&d, 5 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(d, 0, 5 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hrt::launch_math_check_rng(d, nullptr);
  if (e == hipSuccess) e = hipMemcpy(out, d, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (d) (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(nullptr, e, "hrt_debug_math_check_rng");
  return HRT_OK;
}

// Test support: the pair traversal's cross-lane LDS handoffs (hrt_kernels.hip lds_put / lds_get /
// wq_slot_*, wave_handoff) on a scripted run of one wave; the host model is tests/test_gpu_boundary.py's.
extern "C" hrt_status hrt_debug_wq_protocol(int device, uint32_t rounds, const uint32_t* cnt, const uint32_t* take,
                                            const uint32_t* tgt, const uint64_t* val, const uint64_t seed[64],
                                            uint32_t* popped, uint64_t* seen, uint64_t slots[64], uint32_t* depth) {
  if (!cnt || !take || !tgt || !val || !seed || !popped || !seen || !slots || !depth || rounds == 0 || rounds > 1024)
    return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_debug_wq_protocol: bad arguments");
  for (uint32_t i = 0; i < rounds * 64u; ++i)
    if (cnt[i] > 4u) return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_debug_wq_protocol: cnt > 4");
  const size_t nr = (size_t)rounds * 64;
  // device layout: u64 [val nr][seed 64][seen nr][slots 64], then u32 [cnt nr][take rounds][tgt nr][popped nr][depth]
  const size_t b64 = (2 * nr + 128) * 8, b32 = (3 * nr + rounds + 1) * 4;
  char* d = nullptr;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc((void**)&d, b64 + b32);
  unsigned long long* dval = reinterpret_cast<unsigned long long*>(d);
  unsigned long long* dseed = dval + nr;
  unsigned long long* dseen = dseed + 64;
  unsigned long long* dslots = dseen + nr;
  uint32_t* dcnt = reinterpret_cast<uint32_t*>(d + b64);
  uint32_t* dtake = dcnt + nr;
  uint32_t* dtgt = dtake + rounds;
  uint32_t* dpop = dtgt + nr;
  uint32_t* ddepth = dpop + nr;
  if (e == hipSuccess) e = hipMemset(d, 0, b64 + b32);
  if (e == hipSuccess) e = hipMemcpy(dval, val, nr * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dseed, seed, 64 * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dcnt, cnt, nr * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dtake, take, rounds * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dtgt, tgt, nr * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hrt::launch_wq_protocol_check(rounds, dcnt, dtake, dtgt, dval, dseed, dpop, dseen, dslots, ddepth, nullptr);
  if (e == hipSuccess) e = hipMemcpy(popped, dpop, nr * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(seen, dseen, nr * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(slots, dslots, 64 * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(depth, ddepth, 4, hipMemcpyDeviceToHost);
  if (d) (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(nullptr, e, "hrt_debug_wq_protocol");
  return HRT_OK;
}

// Test support: the band lists' wave flattening (hrt_kernels.hip BandFlat) on 64 given lists;
// owner_entry[(r * 64 + l) * 2 + {0, 1}] = owner lane and entry of slot r * 64 + l, r < rounds.
extern "C" hrt_status hrt_debug_band_flatten(int device, const uint32_t n[64], const uint32_t b0[64], uint32_t rounds,
                                             uint32_t* owner_entry, uint32_t* total) {
  if (!n || !b0 || !owner_entry || !total || rounds == 0 || rounds > 4096)
    return fail(nullptr, HRT_ERR_INVALID_ARGUMENT, "hrt_debug_band_flatten: bad arguments");
  uint32_t* d = nullptr;
  const size_t words = 128 + (size_t)rounds * 128 + 1;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc((void**)&d, words * 4);
  if (e == hipSuccess) e = hipMemcpy(d, n, 64 * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + 64, b0, 64 * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hrt::launch_band_flatten_check(d, d + 64, rounds, d + 128, nullptr);
  if (e == hipSuccess) e = hipMemcpy(owner_entry, d + 128, (size_t)rounds * 128 * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(total, d + 128 + (size_t)rounds * 128, 4, hipMemcpyDeviceToHost);
  if (d) (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(nullptr, e, "hrt_debug_band_flatten");
  return HRT_OK;
}

extern "C" hrt_status hrt_debug_unmap_memory(void* ptr, uint64_t size) {
  if (hipMemUnmap(ptr, size) != hipSuccess || hipMemAddressFree(ptr, size) != hipSuccess) return HRT_ERR_HIP;
  return HRT_OK;
}

extern "C" hrt_status hrt_read_rays(hrt_context* ctx, hrt_ray* out, uint32_t n) {
  if (!ctx || (!out && n) || (uint64_t)n > ctx->n_rays || !ctx->scene.rays)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_read_rays: no rays or n too large");
  hrt_status st = hrt_synchronize(ctx);
  if (st != HRT_OK) return st;
  if (n) HRT_HIP(ctx, hipMemcpy(out, ctx->scene.rays, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
  return HRT_OK;
}

extern "C" hrt_status hrt_get_tile_profile(hrt_context* ctx, uint64_t* out, uint32_t count) {
  if (!ctx || !out || count > 4 * ctx->num_tiles() || !ctx->tile_cycles)
    return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_get_tile_profile: needs HRT_OPT_COUNTERS = 2 and a trace");
  hrt_status st = hrt_synchronize(ctx);
  if (st != HRT_OK) return st;
  HRT_HIP(ctx, hipMemcpy(out, ctx->tile_cycles, (size_t)count * 8, hipMemcpyDeviceToHost));
  return HRT_OK;
}

extern "C" hrt_status hrt_get_scene_info(hrt_context* ctx, uint32_t* out, uint32_t count) {
  if (!ctx || !out || count > HRT_NUM_SCENE_INFO) return HRT_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < count; ++i) out[i] = ctx->scene.bvh_info[i];
  return HRT_OK;
}

extern "C" hrt_status hrt_reset_stats(hrt_context* ctx) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = hrt_synchronize(ctx);
  if (st != HRT_OK) return st;
  if ((st = harvest_events(ctx)) != HRT_OK) return st;
  HRT_HIP(ctx, hipMemsetAsync(ctx->counters, 0, hrt::kNumCounters * sizeof(unsigned long long), ctx->stream));
  HRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->traces = ctx->accumulates = 0;
  ctx->last_ms = ctx->total_ms = 0.0f;
  return HRT_OK;
}

extern "C" hrt_status hrt_set_option(hrt_context* ctx, uint32_t key, int64_t value) {
  if (!ctx) return HRT_ERR_INVALID_ARGUMENT;
  switch (key) {
    case HRT_OPT_KERNEL_VARIANT:
      if (value < HRT_KERNEL_AUTO || value > HRT_KERNEL_BUNDLE_WQ_L2)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "kernel variant must be an hrt_kernel value (0..10)");
      if (value == HRT_KERNEL_BUNDLE_WQ_L2)  // its node image, unless the scene's is already on the device
        if (hrt_status st = upload_wq_bfs(ctx); st != HRT_OK) return st;
      ctx->variant = (int)value;
      return HRT_OK;
    case HRT_OPT_COUNTERS:
      if (value < 0 || value > 2) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "counters option must be 0, 1 or 2");
      if (value == 2 && !ctx->tile_cycles) {  // allocated here, so that hrt_trace never allocates
        hrt_status st = hrt_synchronize(ctx);
        if (st != HRT_OK) return st;
        HRT_HIP(ctx, hrt::dev_alloc(ctx, (void**)&ctx->tile_cycles,
                               std::max<size_t>(ctx->num_tiles(), 1) * 4 * sizeof(unsigned long long)));
      }
      ctx->counters_on = value != 0;
      ctx->diag_on = value == 2;
      return HRT_OK;
    case HRT_OPT_SECONDARY_BATCH:
      if (value < 0 || value > 64)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "secondary batch must be 0 (auto) or in [1, 64]");
      ctx->sec_batch = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_PRIMARY_BATCH:
      if (value < 0 || value > 64)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "primary batch must be 0 (auto) or in [1, 64]");
      ctx->prim_batch = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_SPLIT:
      if (value < 0 || value > 64 || (value & (value - 1)) != 0)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "split must be 0 (auto) or a power of two up to 64");
      ctx->split_k = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_SPLIT_FACTOR:
      if (value < -1 || value > 1000000)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "split factor must be -1 (auto) or 0..1000000");
      ctx->split_factor = (int32_t)value;
      return HRT_OK;
    case HRT_OPT_PRIORITY:
#ifdef HRT_DEBUG_OPTIONS
      if (value < 0 || value > 2) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "priority must be 0, 1 or 2");
#else
      if (value < 0 || value > 1)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT,
                    "priority must be 0 or 1 (2, heavy tiles only, is in libhip_raytrace_debug.so)");
#endif
      ctx->split_prio = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_PROBE:
      if (value != 0 && value != 1) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "probe must be 0 or 1");
      ctx->probe = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_FRAMES_PER_LAUNCH:
      if (value < 1 || value > 1024)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "frames per launch must be in [1, 1024]");
      ctx->frames_per_launch = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_OVERLAP:
      if (value < 0 || value > hrt::kLanes)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "overlap must be 0..3 trace lanes (0 and 1: one lane)");
      ctx->overlap = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_BUSY_SPLIT:
      if (value < 1 || value > 8) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "busy split must be in [1, 8]");
      ctx->busy_split = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_WQ_NODE_CAP:
      if (value != 0 && (value < 128 || value > (1 << 20)))
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "wq node cap must be 0 (auto) or in [128, 2^20]");
      ctx->wq_node_cap = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_COOP:
      if (value != 0 && value != 1) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "coop must be 0 or 1");
      ctx->coop = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_BVH_WIDTH:
      if (value < 2 || value > (int64_t)hrt::kWqMaxWidth)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "BVH width must be in [2, 4]");
      ctx->bvh_width = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_WQ_NODE_RADIUS:
      if (value < 0 || value > 2) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "wq node radius must be 0 (auto), 1 or 2");
      ctx->wq_node_radius = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_WQ_LDS_NODES:
      if (value < -1 || value > (1 << 20))
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "wq lds nodes must be -1 (auto) or in [0, 2^20]");
      ctx->wq_lds_nodes = (int32_t)value;
      return HRT_OK;
    case HRT_OPT_SKY_LANE:
      if (value < -1 || value > 1) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "sky lane must be -1 (auto), 0 or 1");
      ctx->sky_lane = (int32_t)value;
      return HRT_OK;
    case HRT_OPT_DEFER_COMBINE: {
      if (value < 0 || value > 1) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "defer combine must be 0 or 1");
      hrt_status st = bind(ctx);
      if (st == HRT_OK) st = hrt::flush_combines(ctx);
      if (st != HRT_OK) return st;
      ctx->defer = (uint32_t)value;
      return HRT_OK;
    }
    case HRT_OPT_FOLD_RECORDS: {
      if (value < 0 || value > 1) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "fold records must be 0 or 1");
      hrt_status st = bind(ctx);
      if (st == HRT_OK) st = hrt::flush_combines(ctx);  // (combines deferred so far fold under the old setting)
      if (st != HRT_OK) return st;
      if (value == 1 && !ctx->fold_ring)  // allocated here, so that no fold allocates
        HRT_HIP(ctx, hrt::dev_alloc(ctx, (void**)&ctx->fold_ring, HRT_FOLD_RECORD_RING * sizeof(hrt_fold_record)));
      if (value == 1) ctx->fold_frame.assign(HRT_FOLD_RECORD_RING, 0u);
      ctx->fold_total = 0;  // the ring is empty: a slot is zeroed before the fold that uses it
      ctx->fold_on = (uint32_t)value;
      return HRT_OK;
    }
    case HRT_OPT_COMM_TIMEOUT_MS:
      if (value < 0 || value > 0xFFFFFFFFll)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "comm timeout must be in [0, 2^32) ms (0 = wait forever)");
      ctx->comm_timeout_ms = (uint32_t)value;
      return HRT_OK;
    case HRT_OPT_BVH_LEAF_SIZE:
      if (value < 0 || value > hrt::kBvhMaxLeafCount)
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "BVH leaf size must be 0 (auto) or in [1, 16]");
      ctx->bvh_leaf = (uint32_t)value;
      return HRT_OK;
#ifdef HRT_DEBUG_OPTIONS
    case HRT_OPT_GRID_CUS:
      if (value < 0) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "grid CUs must be >= 0");
      ctx->grid_cus = (uint32_t)value;
      return HRT_OK;
    case HRT_DEBUG_OPT_FAIL_ALLOC:
      if (value < 0) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "fail-alloc index must be >= 0");
      ctx->debug_fail_alloc = value;
      return HRT_OK;
    case HRT_DEBUG_OPT_WQ_TRI_CAP:
      if (value != 0 && (value < 128 || value > (1 << 20)))
        return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "wq tri cap must be 0 (auto) or in [128, 2^20]");
      ctx->debug_wq_tri_cap = (uint32_t)value;
      return HRT_OK;
    case HRT_DEBUG_OPT_GRAB_RUNS:
      if (value < 0 || value > 1) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "grab runs must be 0 or 1");
      ctx->debug_grab_runs = (uint32_t)value;
      return HRT_OK;
    case HRT_DEBUG_OPT_STACK_LIMIT:
      if (value < 0) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "stack limit must be >= 0");
      ctx->debug_stack_limit = value;
      ctx->frame_stack_failed = 0;
      return HRT_OK;
#else
    case HRT_OPT_GRID_CUS:
    case HRT_DEBUG_OPT_FAIL_ALLOC:
    case HRT_DEBUG_OPT_WQ_TRI_CAP:
    case HRT_DEBUG_OPT_GRAB_RUNS:
    case HRT_DEBUG_OPT_STACK_LIMIT:
      return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "debug option: only libhip_raytrace_debug.so accepts it");
#endif
    case HRT_DEBUG_OPT_TIMELINE:
#if HRT_TIMELINE
      if (value <= 0 || value > (1 << 24)) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "timeline capacity in [1, 2^24]");
      if (ctx->timeline) {
        HRT_HIP(ctx, hipDeviceSynchronize());  // (every lane's stream: a launch may still be recording)
        free_dev(ctx, ctx->timeline);
        free_dev(ctx, ctx->timeline_count);
      }
      HRT_HIP(ctx, hrt::dev_alloc(ctx, (void**)&ctx->timeline, (size_t)value * 4 * sizeof(unsigned long long)));
      HRT_HIP(ctx, hrt::dev_alloc(ctx, (void**)&ctx->timeline_count, sizeof(uint32_t)));
      HRT_HIP(ctx, hipMemset(ctx->timeline_count, 0, sizeof(uint32_t)));
      ctx->timeline_cap = (uint32_t)value;
      return HRT_OK;
#else
      return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "timeline option: only builds with -DHRT_TIMELINE=1 accept it");
#endif
    default:
      return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "unknown option key");
  }
}

// Test / tuning support (HRT_TIMELINE builds): the last trace launch's per-item records.
extern "C" hrt_status hrt_debug_timeline(hrt_context* ctx, uint64_t* out, uint32_t cap, uint32_t* count) {
  if (!ctx || !out || !count) return HRT_ERR_INVALID_ARGUMENT;
  if (!ctx->timeline) return fail(ctx, HRT_ERR_INVALID_ARGUMENT, "hrt_debug_timeline: HRT_DEBUG_OPT_TIMELINE not set");
  if (bind(ctx) != HRT_OK) return HRT_ERR_HIP;
  HRT_HIP(ctx, hipDeviceSynchronize());
  uint32_t n = 0;
  HRT_HIP(ctx, hipMemcpy(&n, ctx->timeline_count, sizeof n, hipMemcpyDeviceToHost));
  n = std::min(n, ctx->timeline_cap);
  *count = n;
  HRT_HIP(ctx, hipMemcpy(out, ctx->timeline, (size_t)std::min(n, cap) * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return HRT_OK;
}

// Test support: the tile_lists kernel's records for a dispatch of pc, built into a buffer of the call's own
// (the lanes' tl_cache records stay what the last launch made them) from lane 0's camera lists, which the
// call rebuilds for pc's camera -- so lane 0's next trace rebuilds both.  Per tile: n, ok, then the listed
// triangles' indices into the uploaded buffer (cam_tris[..][1].w of each entry's record).
extern "C" hrt_status hrt_debug_tile_lists(hrt_context* ctx, const hrt_push_constants* pc, uint32_t refine,
                                           uint32_t* out, uint64_t words, uint32_t info[2]) {
  if (!ctx || !pc || !info) return HRT_ERR_INVALID_ARGUMENT;
  hrt_status st = bind(ctx);
  if (st != HRT_OK) return st;
  if ((st = check_dispatch(ctx, pc, "hrt_debug_tile_lists")) != HRT_OK) return st;
  constexpr uint32_t kWords = 66;
  const uint32_t tiles = (uint32_t)ctx->num_tiles();
  info[0] = tiles;
  info[1] = (ctx->width + 7) / 8;
  if (!out || words < (uint64_t)tiles * kWords) return HRT_OK;
  if ((st = hrt_synchronize(ctx)) != HRT_OK) return st;
  hrt::TraceParams p = make_params(ctx, pc, 0);
  uint32_t* recs = nullptr;
  HRT_HIP(ctx, hipMalloc((void**)&recs, (size_t)tiles * hrt::kTlRecWords * 4));
  p.tl_cache = recs;
  ctx->lane[0].cam_ready = ctx->lane[0].tl_ready = false;
  hipError_t e = hrt::launch_tile_lists(p, refine, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  std::vector<uint32_t> host((size_t)tiles * hrt::kTlRecWords);
  const size_t cap = ctx->scene.cam_capacity;
  std::vector<float> cam(cap * 16);
  if (e == hipSuccess) e = hipMemcpy(host.data(), recs, host.size() * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && cap) e = hipMemcpy(cam.data(), ctx->scene.cam_tris[0], cam.size() * 4, hipMemcpyDeviceToHost);
  (void)hipFree(recs);
  if (e != hipSuccess) return hip_fail(ctx, e, "hrt_debug_tile_lists");
  for (uint32_t t = 0; t < tiles; ++t) {
    const uint32_t* rec = &host[(size_t)t * hrt::kTlRecWords];
    uint32_t* o = out + (size_t)t * kWords;
    const uint32_t n = std::min(rec[128], 64u);
    o[0] = n;
    o[1] = rec[129];
    for (uint32_t i = 0; i < 64; ++i) {
      const size_t k = rec[i] & 0x07FFFFFFu;
      uint32_t idx = 0xFFFFFFFFu;
      if (i < n && k < cap) std::memcpy(&idx, &cam[k * 16 + 7], 4);
      o[2 + i] = idx;
    }
  }
  return HRT_OK;
}

// Work the caller enqueues on the stream follows every accumulate so far: the deferred ones are folded.
extern "C" void* hrt_stream(hrt_context* ctx) {
  if (!ctx || bind(ctx) != HRT_OK || hrt::flush_combines(ctx) != HRT_OK) return ctx ? (void*)ctx->stream : nullptr;
  return (void*)ctx->stream;
}

extern "C" hrt_status hrt_release_caches(uint64_t* freed_bytes) {
  const uint64_t bytes = hrt::release_band_cache();
  if (freed_bytes) *freed_bytes = bytes;
  return HRT_OK;
}

extern "C" const char* hrt_last_error(const hrt_context* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}
