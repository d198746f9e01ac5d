/*
 * hip_raytrace.h -- C ABI of libhip_raytrace.so, the MI355X (gfx950) drop-in for the compute side
 * of hindlet/EPQ_Raytracer: the path-trace dispatch (assets/raytracing.glsl) and the progressive
 * frame accumulator (assets/image_combiner.glsl).
 *
 * What each entry point replaces (reference paths relative to the reference repo root):
 *   hrt_create       RayTracePipeline::new      src/raytrace_pipeline.rs:51-97   (pipeline + R8G8B8A8 image :67-73)
 *                    DiffusePipeline::new       src/diffuse.rs:35-66             (accumulated image :50-56)
 *   hrt_set_scene    create_ray_subbuffer / create_sphere_subbuffer / create_mesh_subbuffer uploads
 *                                               src/raytrace_pipeline.rs:75-77, :302, :337, :349, :359, :371-372
 *   hrt_trace        RayTracePipeline::compute  src/raytrace_pipeline.rs:162-187 (pc->init == 0)
 *                    RayTracePipeline::init     src/raytrace_pipeline.rs:190-213 (pc->init != 0)
 *                    -> dispatch + push constants  src/raytrace_pipeline.rs:216-266
 *   hrt_accumulate   DiffusePipeline::next_frame src/diffuse.rs:73-101 (-> dispatch :103-136)
 *   hrt_read_image   RayTracePipeline::image / DiffusePipeline::image  src/raytrace_pipeline.rs:156, src/diffuse.rs:69
 *                    (on a row-tile partition with a communicator: the RCCL framebuffer gather, hrt_comm_*)
 *   hrt_present      RenderPassOverFrame::render src/texture_draw_pipeline.rs:96-157 (the accumulated image as a
 *                    nearest-sampled, vertically flipped quad over the B8G8R8A8_UNORM target, src/raytracing_app.rs:104-109)
 *   hrt_synchronize  then_signal_fence_and_flush().unwrap() + fence wait  src/raytrace_pipeline.rs:179-183
 *   hrt_last_error   the .unwrap() panics (every Vulkan call in src/raytrace_pipeline.rs / src/diffuse.rs)
 *
 * Records are byte-identical to the GLSL std430 structs (assets/raytracing.glsl:51-111) and the
 * 124-byte push-constant block (assets/raytracing.glsl:135-153, src/raytrace_pipeline.rs:125-139),
 * so a Rust caller can pass its raytrace_shader::* slices verbatim.
 *
 * Conventions: every function returns hrt_status (0 = OK).  No exceptions cross the ABI.  Host
 * arrays are borrowed for the duration of the call only.  A context is NOT thread-safe: use it from
 * one host thread.  All work on a context is ordered on the context's own HIP stream
 * (== the reference's GpuFuture chaining); hrt_trace / hrt_accumulate return without waiting.
 * Internally a trace runs on one of three trace lanes (own stream + trace image) so that frame k+1's
 * trace overlaps frame k's tail; the combiner, reads and every other call stay in call order on the
 * context's stream, so results equal the serial loop's byte for byte (HRT_OPT_OVERLAP).
 */
#ifndef HIP_RAYTRACE_H
#define HIP_RAYTRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6, additive (no bump: nothing existing changed): object motion in the temporal history -- HRT_MOTION_MOVING,
 * HRT_MOTION_MAX_OBJECTS, HRT_MOTION_RING, hrt_motion, hrt_motion_tables, hrt_reproject_motion,
 * hrt_reproject_motion_moments (and hrt_host_motion_between in hrt_host.h).
 * 6, additive (no bump: nothing existing changed): temporal upsampling -- HRT_RESOLVE_FILL, HRT_RESOLVE_MOMENTS,
 * hrt_resolve_info, hrt_resolve_defaults, hrt_set_ray_grid, hrt_history_phase, hrt_accumulate_history_from.
 * 6, additive (no bump: nothing existing changed): guided upsampling -- HRT_UPSAMPLE_FOOTPRINT, hrt_upsample_info,
 * hrt_upsample_defaults, hrt_upsample, hrt_upsample_present, hrt_order_after.
 * 6, additive (no bump: nothing existing changed): tile-masked refinement -- HRT_REFINE_TILES_MAX_FRAMES,
 * hrt_refine_tiles_stats, hrt_refine_tiles, hrt_refine_tiles_until.
 * 6, additive (no bump: nothing existing changed): adaptive refinement -- hrt_refine_rule, hrt_refine_method,
 * HRT_REFINE_MOMENTS, hrt_refine_stats, hrt_refine_defaults, hrt_refine_select, hrt_refine, hrt_refine_until.
 * 6, additive (no bump: nothing existing changed): the variance-guided denoise -- hrt_variance_method,
 * hrt_variance_info, hrt_variance_defaults, hrt_accumulate_history_moments, hrt_reproject_moments, hrt_fill_moments,
 * hrt_read_moments, hrt_denoise_variance, hrt_denoise_variance_present.
 * 6, additive (no bump: nothing existing changed): the first-hit pass -- hrt_first_hits_method,
 * HRT_FIRST_HITS_COUNT, hrt_first_hits_stats, hrt_first_hits, hrt_get_first_hits_stats.
 * 6, additive (no bump: nothing existing changed): temporal history -- hrt_view, hrt_reproject_filter,
 * hrt_reproject_info, hrt_reproject_defaults, hrt_reproject, hrt_accumulate_history, hrt_fill_history,
 * hrt_read_history.
 * 6, additive (no bump: nothing existing changed): the denoise pass -- hrt_denoise_method, hrt_denoise_info,
 * hrt_denoise_defaults, hrt_denoise, hrt_denoise_present.
 * 6, additive (no bump: nothing existing changed): radiance queries -- hrt_radiance_query, hrt_radiance_stats,
 * hrt_radiance.
 * 6, additive (no bump: nothing existing changed): occlusion queries -- hrt_occlusion_stats, hrt_occluded.
 * 6, additive (no bump: nothing existing changed): HRT_KERNEL_BUNDLE_WQ_L2, HRT_OPT_WQ_LDS_NODES,
 * hrt_debug_bvh_wq_nodes_bfs, hrt_debug_wq_l2_plan.
 * 6, additive (no bump: nothing existing changed): ray queries -- hrt_ray_query, hrt_hit, hrt_query_stats,
 * hrt_query_method, hrt_intersect, hrt_intersect_primary.
 * 6, additive (no bump: nothing existing changed): hrt_debug_tile_lists.
 * 6, additive (no bump: nothing existing changed): HRT_OPT_SKY_LANE, hrt_debug_sky_units.
 * 6, additive (no bump: nothing existing changed): fold records -- hrt_fold_record, hrt_settle_rule,
 * HRT_OPT_FOLD_RECORDS, hrt_get_fold_records, hrt_compute_until, HRT_FOLD_RECORD_RING, HRT_RGBA8_FREEZE_FRAME.
 * 6, additive (no bump: nothing existing changed): the present pass -- hrt_present_format,
 * hrt_present_info, hrt_present, hrt_accumulate_present, hrt_present_done, hrt_present_wait.
 * 6, additive (no bump: nothing existing changed; hrt_get_diagnostics takes the caller's count):
 * HRT_OPT_PRIMARY_BATCH, HRT_DIAG_PRIMARY_DEFERRED, HRT_DIAG_BATCH_ONLY_ITERS (HRT_NUM_DIAG 32).
 * 6, additive (no bump: hrt_get_diagnostics takes the caller's count): HRT_DIAG_DIR_LANES (HRT_NUM_DIAG 30).
 * 6 (r06): hrt_release_caches; HRT_DEBUG_OPT_STACK_LIMIT.
 * 5 (r05): HRT_DIAG_WQ_STEPS_* / WQ_MEMBERS (HRT_NUM_DIAG 29), HRT_DEBUG_OPT_TIMELINE + hrt_debug_timeline.
 * 4 (r04): hrt_debug_wq_protocol; hrt_stats.last_frames; HRT_DIAG_SKY_* / PRIMARY_LANES / LOOP_ITERS /
 * LIVE_LANES (HRT_NUM_DIAG 24).
 * 3 (r03): hrt_debug_band_flatten.
 * 2 (r03): HRT_ERR_COMM, HRT_IMG_LOCAL, HRT_OPT_COMM_TIMEOUT_MS, collective error agreement;
 * hrt_debug_bvh_wq_nodes' width parameter; HRT_NUM_DIAG / HRT_NUM_SCENE_INFO grown (r02). */
#define HRT_ABI_VERSION 6u

typedef enum hrt_status {
  HRT_OK = 0,
  HRT_ERR_INVALID_ARGUMENT = 1, /* bad pointer / size / count / push-constant field */
  HRT_ERR_NO_DEVICE = 2,        /* no HIP device, or the requested ordinal does not exist */
  HRT_ERR_OUT_OF_MEMORY = 3,
  HRT_ERR_NO_SCENE = 4,         /* hrt_trace before hrt_set_scene */
  HRT_ERR_HIP = 5,              /* a HIP runtime call failed; hrt_last_error has the text */
  HRT_ERR_IO = 6,               /* file not found / unparsable (host helpers) */
  HRT_ERR_COMM = 7              /* a collective (hrt_comm_init, hrt_read_image on a joined context) failed
                                   on ANOTHER rank, timed out or was aborted; every rank of the call
                                   returns an error and none is left blocked (hrt_comm.cpp) */
} hrt_status;

/* ---- std430 records (assets/raytracing.glsl:51-111) ---------------------------------------- */

/* RayTracingMaterial, raytracing.glsl:51-55.  settings = (specular probability, metallic, fuzz,
 * invisible flag == 1.0).  Built by src/materials.rs:13-94. */
typedef struct hrt_material {
  float colour[4];
  float emission[4]; /* rgb, strength */
  float settings[4];
} hrt_material;

/* Ray, raytracing.glsl:66-68: camera-space sample centre around (1,0,0) (w unused). */
typedef struct hrt_ray {
  float sample_centre[4];
} hrt_ray;

/* Sphere, raytracing.glsl:71-75 */
typedef struct hrt_sphere {
  float centre[3];
  float radius;
  hrt_material material;
} hrt_sphere;

/* Triangle, raytracing.glsl:79-84 (w components unused) */
typedef struct hrt_triangle {
  float a[4];
  float edge_one[4]; /* b - a */
  float edge_two[4]; /* c - a */
  float normal[4];   /* edge_one x edge_two, NOT normalised */
} hrt_triangle;

/* Mesh, raytracing.glsl:87-93: triangles[first_index .. first_index+len) */
typedef struct hrt_mesh {
  float min_point[3];
  uint32_t first_index;
  float max_point[3];
  uint32_t len;
  hrt_material material;
} hrt_mesh;

/* PushConstants, raytracing.glsl:135-153 (std430, 124 bytes) */
typedef struct hrt_push_constants {
  float cam_pos[4];
  float cam_alignment_mat[16]; /* column-major mat4; mat3(M) is used */
  int32_t num_rays;
  int32_t num_spheres;
  int32_t num_meshes;
  int32_t num_samples;
  float jitter_size;
  int32_t max_bounces;
  uint32_t use_environment_light; /* GLSL bool */
  uint32_t rng_offset;
  uint32_t init; /* GLSL bool: 1 -> clear the trace image to (0,0,0,1) */
  uint32_t width;
  uint32_t height;
} hrt_push_constants;

/* ---- context ------------------------------------------------------------------------------ */

typedef enum hrt_mode {
  HRT_MODE_RGBA8 = 0,  /* reference-faithful: trace + accumulator images are R8G8B8A8_UNORM */
  HRT_MODE_RGBA32F = 1 /* fp32 images, same arithmetic without the per-frame 8-bit requantization */
} hrt_mode;

typedef enum hrt_image_id {
  HRT_IMG_TRACE = 0,
  HRT_IMG_ACCUM = 1,
  /* flag, OR-ed with one of the above: this context's LOCAL rows even when it is joined to a
   * communicator -- not a collective (checkpoints of a partition, per-rank inspection) */
  HRT_IMG_LOCAL = 0x100
} hrt_image_id;
typedef enum hrt_format { HRT_FMT_RGBA8 = 0, HRT_FMT_RGBA32F = 1 } hrt_format;

typedef struct hrt_create_info {
  uint32_t width;      /* full image size (image_size[0]) */
  uint32_t height;     /* image_size[1] */
  int32_t device;      /* HIP device ordinal; -1 = the calling thread's current device */
  uint32_t mode;       /* hrt_mode */
  /* Image-space partition (multi-GPU row tiles).  Rows are grouped into tiles of
   * row_tile rows; this context renders tiles t with t % part_count == part_index and stores them
   * compacted (local row r <-> global row ((r / row_tile) * part_count + part_index) * row_tile
   * + r % row_tile).  part_count == 0 or 1 means the whole image. */
  uint32_t row_tile;
  uint32_t part_index;
  uint32_t part_count;
} hrt_create_info;

typedef struct hrt_layout {
  uint32_t width, height;   /* full image */
  uint32_t local_rows;      /* rows stored by this context (padded: equal on every part) */
  uint32_t row_tile, part_index, part_count;
  uint32_t mode;
} hrt_layout;

typedef struct hrt_stats {
  uint64_t segments;      /* world_hit calls (raytracing.glsl:317) over all traces since reset */
  uint64_t tri_tests;     /* ray-triangle tests (Sum over AABB-passing meshes of len) since reset */
  uint64_t traces;        /* non-init trace dispatches since reset */
  uint64_t accumulates;   /* combiner dispatches since reset */
  float last_trace_ms;    /* device time of the last trace dispatch (HIP events) */
  float total_trace_ms;   /* device time of all trace dispatches since reset */
  uint64_t wave_steps;    /* sum over work items of the item's longest per-lane segment count: lane
                             efficiency = segments / (64 * wave_steps).  A frame run of a multi-frame
                             launch (hrt_compute_n) is one item: each lane's segments summed over the
                             run's pixel-frames it took (any pixel of the tile), so the figure is
                             comparable between launches of the same shape only */
  uint32_t last_kernel;   /* hrt_kernel the last trace ran (HRT_KERNEL_AUTO resolved) */
  uint32_t last_block;    /* its workgroup size (threads) */
  uint32_t last_frames;   /* frames the last trace launch held (hrt_compute_n packs up to
                             HRT_OPT_FRAMES_PER_LAUNCH into one launch; 1 for hrt_trace) (ABI 4) */
  uint32_t reserved;
} hrt_stats;

/* The present pass (hrt_present): the byte order of a target pixel. */
typedef enum hrt_present_format {
  HRT_PRESENT_B8G8R8A8 = 0, /* the reference's swapchain format (src/raytracing_app.rs:104-109) */
  HRT_PRESENT_R8G8B8A8 = 1  /* the image's own byte order */
} hrt_present_format;

/* The target of one present pass: width x height pixels of 4 bytes, rows pitch bytes apart. */
typedef struct hrt_present_info {
  uint32_t image_id;      /* HRT_IMG_ACCUM or HRT_IMG_TRACE */
  uint32_t format;        /* hrt_present_format */
  uint32_t width, height; /* target size in pixels, each 1..16384 */
  uint32_t pitch;         /* bytes per target row: >= width*4, a multiple of 4 */
  uint32_t flags;         /* must be 0 */
} hrt_present_info;

/* ---- fold records (HRT_OPT_FOLD_RECORDS, hrt_get_fold_records, hrt_compute_until) ----
 * The displayed word D(p) of an accumulator pixel: in HRT_MODE_RGBA8 the accumulator's 32-bit word; in
 * HRT_MODE_RGBA32F the RGBA8 word hrt_read_image(HRT_FMT_RGBA8) and the present pass make of it.  The
 * record of one fold (one frame folded into the accumulator) is taken over the context's REAL pixels: its
 * local rows whose global row is below height (the padding rows of a row-tile part are never counted). */
#define HRT_FOLD_RECORD_RING 1024u   /* records kept per context */
#define HRT_RGBA8_FREEZE_FRAME 510u  /* HRT_MODE_RGBA8: a fold with frame >= this changes no pixel, whatever the new frame holds */

typedef struct hrt_fold_record {
  uint32_t frame;          /* the frame number the fold was given */
  uint32_t changed_pixels; /* pixels with D before != D after */
  uint32_t max_delta;      /* the largest |byte after - byte before| over the four bytes of every pixel */
  uint32_t reserved;       /* 0 */
  uint64_t abs_delta_sum;  /* the sum of |byte after - byte before| over the four bytes of every pixel */
} hrt_fold_record;

typedef struct hrt_settle_rule {
  uint32_t max_changed_pixels; /* a frame is quiet when its record has changed_pixels <= this ... */
  uint32_t max_delta;          /* ... and max_delta <= this (0xFFFFFFFF disables either bound) */
  uint32_t quiet_frames;       /* stop after this many consecutive quiet frames of THIS call; >= 1 */
  uint32_t flags;              /* must be 0 */
} hrt_settle_rule;

/* ---- ray queries (hrt_intersect, hrt_intersect_primary) ---- */
typedef struct hrt_ray_query {
  float origin[3];
  float t_max;        /* the running closest starts at min(t_max, FLT_MAX); NaN or <= 0.001: a certain miss */
  float direction[3]; /* any length: normalised by S4 before the scan; t is along the normalised direction */
  uint32_t reserved;  /* ignored */
} hrt_ray_query;

typedef struct hrt_hit {
  float t;           /* the reference's hit_dist; FLT_MAX for a miss */
  uint32_t kind;     /* 0 miss, 1 sphere, 2 triangle */
  uint32_t index;    /* sphere index / index into the uploaded triangle buffer; 0xFFFFFFFF for a miss */
  uint32_t mesh;     /* mesh index of a triangle hit; 0xFFFFFFFF otherwise */
  float normal[3];   /* the reference's hit normal (unit, not flipped toward the ray); 0 for a miss */
  uint32_t reserved; /* 0 */
} hrt_hit;

typedef struct hrt_query_stats {
  uint32_t method_ran; /* hrt_query_method that ran: AUTO resolved, fallbacks applied */
  uint32_t reserved;   /* 0 */
  uint64_t scan_rays;  /* rays answered by the literal scan because their origin or normalised direction is not finite */
  uint64_t tri_tests;  /* sum over rays of len of every mesh whose AABB test passes (hrt_stats.tri_tests per segment) */
} hrt_query_stats;

typedef enum hrt_query_method {
  HRT_QUERY_AUTO = 0,  /* BVH when the hierarchy is built, else SCAN */
  HRT_QUERY_SCAN = 1,  /* the reference's scan, statement by statement */
  HRT_QUERY_BVH = 2,   /* per-lane traversal of the global-memory hierarchy (SCAN when it was not built) */
  HRT_QUERY_PAIRS = 3  /* the pair traversal, 64 rays per wave (BVH when its node image does not fit) */
} hrt_query_method;

/* ---- occlusion queries (hrt_occluded) ---- */
typedef struct hrt_occlusion_stats {
  uint32_t method_ran; /* as hrt_query_stats */
  uint32_t reserved;   /* 0 */
  uint64_t scan_rays;  /* as hrt_query_stats */
  uint64_t tri_tests;  /* as hrt_query_stats: the sum over live rays of len of every mesh whose AABB test passes --
                          by definition, whatever the traversal skipped after a hit */
  uint64_t occluded;   /* rays whose bit is 1 */
} hrt_occlusion_stats;

/* ---- radiance queries (hrt_radiance) ---- */
typedef struct hrt_radiance_query { /* 32 bytes, two 16-byte loads */
  float origin[3];   /* trace_ray's root */
  uint32_t seed;     /* the RNG state main() would start the pixel with */
  float centre[3];   /* the sample centre get_ray_dir jitters and rotates */
  uint32_t reserved; /* ignored */
} hrt_radiance_query;

typedef struct hrt_radiance_stats {
  uint32_t method_ran;    /* as hrt_query_stats */
  uint32_t reserved;      /* 0 */
  uint64_t scan_segments; /* segments answered by the literal scan because they are irregular (S11's rule, per
                             segment: origin not finite, or direction not finite, or its dot(d, d) zero, denormal
                             or overflowed) */
  uint64_t segments;      /* world_hit calls, as hrt_stats.segments counts them */
  uint64_t tri_tests;     /* as hrt_stats.tri_tests */
} hrt_radiance_stats;

/* ---- the denoise pass (hrt_denoise, hrt_denoise_present) ---- */
typedef enum hrt_denoise_method {
  HRT_DENOISE_AUTO = 0,   /* per step, the kernel that measured faster */
  HRT_DENOISE_DIRECT = 1, /* atrous_direct: every tap a global load */
  HRT_DENOISE_TILED = 2   /* atrous_tiled: taps from a tile staged in LDS */
} hrt_denoise_method;
/* libhip_raytrace_debug.so only (measurements of the tiled kernel's two forms): the dense tile
 * at every step whose halo fits (1, 2, 4; the sub-lattice above), and the sub-lattice at every step */
#define HRT_DEBUG_DENOISE_DENSE 3u
#define HRT_DEBUG_DENOISE_LATTICE 4u
/* hrt_denoise_defaults' sigmas: design parameters chosen on the CPU oracle's frames */
#define HRT_DENOISE_SIGMA_COLOUR 8.0f
#define HRT_DENOISE_SIGMA_NORMAL 0.25f
#define HRT_DENOISE_SIGMA_DEPTH 0.5f

typedef struct hrt_denoise_info { /* 32 bytes */
  uint32_t image_id;   /* HRT_IMG_ACCUM or HRT_IMG_TRACE */
  uint32_t iterations; /* 1..5: passes with steps 1, 2, 4, 8, 16 */
  uint32_t method;     /* hrt_denoise_method; every method gives the same bytes */
  uint32_t flags;      /* must be 0 */
  float sigma_colour;  /* each sigma finite and > 0 */
  float sigma_normal;
  float sigma_depth;
  uint32_t reserved;   /* ignored */
} hrt_denoise_info;

/* ---- temporal history (hrt_reproject, hrt_accumulate_history) ---- */
/* A view: the camera of a push block plus the affine grid of its ray centres in camera space --
 * the centre of pixel (x, y) is first + dx x + dy y, as hrt_host_ray_grid returns first / px / py. */
typedef struct hrt_view {            /* 128 bytes */
  float cam_pos[4];                  /* as hrt_push_constants */
  float cam_alignment_mat[16];       /* as hrt_push_constants; mat3 used, assumed a rotation */
  float grid_first[4], grid_dx[4], grid_dy[4]; /* w unused */
} hrt_view;

typedef enum hrt_reproject_filter { HRT_REPROJECT_NEAREST = 0, HRT_REPROJECT_BILINEAR = 1 } hrt_reproject_filter;
/* hrt_reproject_defaults' thresholds: design parameters chosen on the CPU oracle's frames */
#define HRT_REPROJECT_DEPTH_TOLERANCE 0.02f
#define HRT_REPROJECT_MIN_NORMAL_DOT 0.9f
#define HRT_HISTORY_MAX 16777216u /* the largest max_history of hrt_accumulate_history: 2^24 */

typedef struct hrt_reproject_info { /* 32 bytes */
  uint32_t filter;       /* hrt_reproject_filter */
  uint32_t flags;        /* must be 0 */
  float depth_tolerance; /* finite, >= 0: a tap is kept when |expected - stored depth| <= tolerance * expected */
  float min_normal_dot;  /* finite: a tap is kept when dot(normal now, normal then) >= this; -2 disables */
  uint32_t reserved[4];  /* ignored */
} hrt_reproject_info;

/* ---- object motion in the temporal history (hrt_reproject_motion) ---- */
#define HRT_MOTION_MOVING 1u          /* hrt_motion.flags bit 0: the object moved between the two frames */
#define HRT_MOTION_MAX_OBJECTS 65536u /* the largest count of either table */
#define HRT_MOTION_RING 4u            /* calls in flight before hrt_reproject_motion waits for the oldest one's pass */
typedef struct hrt_motion { /* 64 bytes */
  float m[12];          /* column-major 3x4 G = [L | b]: previous world point = L * current world point + b;
                           L assumed a rotation (as hrt_view's mat3 is) */
  uint32_t flags;       /* 0: the object did not move (S15's path, untouched); HRT_MOTION_MOVING */
  uint32_t reserved[3]; /* ignored */
} hrt_motion;
typedef struct hrt_motion_tables { /* host arrays, copied before the call returns */
  const hrt_motion* spheres; /* indexed by hrt_hit.index of a kind-1 hit */
  uint32_t n_spheres;
  const hrt_motion* meshes;  /* indexed by hrt_hit.mesh of a kind-2 hit */
  uint32_t n_meshes;
} hrt_motion_tables;

/* ---- the variance-guided denoise (hrt_denoise_variance, the moments calls) ---- */
/* hrt_variance_defaults' parameters: design parameters chosen on the CPU oracle's frames */
#define HRT_VARIANCE_SIGMA 4.0f
#define HRT_VARIANCE_FLOOR 1e-10f
#define HRT_VARIANCE_MIN_HISTORY 4u
typedef enum hrt_variance_method {
  HRT_VARIANCE_AUTO = 0,   /* per step, the kernel that measured faster */
  HRT_VARIANCE_DIRECT = 1, /* atrous_variance_direct: every tap a global load */
  HRT_VARIANCE_TILED = 2   /* atrous_variance_tiled at steps 1, 2, 4: taps from a tile staged in LDS */
} hrt_variance_method;

typedef struct hrt_variance_info { /* 32 bytes */
  uint32_t iterations;  /* 0..5: passes with steps 1, 2, 4, 8, 16; 0 returns the source and the variance estimate */
  uint32_t method;      /* hrt_variance_method; every method gives the same bytes */
  uint32_t flags;       /* must be 0 */
  uint32_t min_history; /* >= 1: counts below it take the spatial estimate */
  float sigma_variance; /* finite, > 0 */
  float variance_floor; /* finite, > 0 */
  float sigma_normal;   /* as hrt_denoise_info */
  float sigma_depth;
} hrt_variance_info;

/* ---- guided upsampling (hrt_upsample, hrt_upsample_present) ---- */
#define HRT_UPSAMPLE_FOOTPRINT 2u /* hrt_upsample_defaults' footprint */
typedef struct hrt_upsample_info { /* 32 bytes */
  uint32_t image_id;  /* HRT_IMG_ACCUM / HRT_IMG_TRACE: the low image; a filter given with it must read the same */
  uint32_t width;     /* the result's and the high guide's size, each 1..16384 */
  uint32_t height;
  uint32_t footprint; /* 2 or 4: the taps per axis */
  uint32_t flags;     /* must be 0 */
  float sigma_normal; /* finite, > 0; as hrt_denoise_info */
  float sigma_depth;
  uint32_t reserved;  /* ignored */
} hrt_upsample_info;

/* ---- temporal upsampling (hrt_accumulate_history_from) ---- */
#define HRT_RESOLVE_FILL 1u    /* a pixel without history that took no sample shows the nearest source texel */
#define HRT_RESOLVE_MOMENTS 2u /* fold the moments image M too */
typedef struct hrt_resolve_info { /* 32 bytes */
  float offset_x;       /* finite, each in [-0.5, 0.5]: source sample i sits at source coordinate i + offset */
  float offset_y;
  uint32_t max_history; /* 1..HRT_HISTORY_MAX, as hrt_accumulate_history */
  uint32_t flags;       /* HRT_RESOLVE_* bits */
  uint32_t reserved[4]; /* ignored */
} hrt_resolve_info;

/* ---- the first-hit pass (hrt_first_hits) ---- */
typedef enum hrt_first_hits_method {
  HRT_FIRST_HITS_AUTO = 0,  /* TILES: it measured faster on island and on cave */
  HRT_FIRST_HITS_TILES = 1, /* first_hits_tiles: one wave per 8x8 tile, the tile's primary triangle list */
  HRT_FIRST_HITS_QUERY = 2  /* the primary query kernel hrt_intersect_primary's AUTO runs, not waited for */
} hrt_first_hits_method;
#define HRT_FIRST_HITS_COUNT 1u /* hrt_first_hits flags bit 0: count on the device (hrt_get_first_hits_stats) */

typedef struct hrt_first_hits_stats { /* 48 bytes: the last call that had HRT_FIRST_HITS_COUNT */
  uint32_t method_ran;      /* hrt_first_hits_method that ran (AUTO resolved) */
  uint32_t reserved;        /* 0 */
  uint32_t tiles;           /* 8x8 tiles of the image (TILES; 0 for QUERY, as the three below and entries_tested) */
  uint32_t tiles_listed;    /* tiles answered from their list */
  uint32_t tiles_empty;     /* listed tiles with no entry and no spheres: stored as misses, no test */
  uint32_t tiles_fallback;  /* tiles whose list was not usable: answered by the per-wave bundle cull */
  uint64_t scan_rays;       /* as hrt_query_stats */
  uint64_t tri_tests;       /* as hrt_query_stats */
  uint64_t entries_tested;  /* list entries that reached the exact test, summed over waves */
} hrt_first_hits_stats;

/* ---- adaptive refinement (hrt_refine_select, hrt_refine, hrt_refine_until) ---- */
/* hrt_refine_defaults' parameters: design parameters chosen on the CPU oracle's frames */
#define HRT_REFINE_TOLERANCE 0.05f
#define HRT_REFINE_RADIUS 1u
#define HRT_REFINE_MIN_HISTORY 4u
#define HRT_REFINE_FLOOR 0.01f
#define HRT_REFINE_MAX_COUNT 16777216u /* 2^24 = HRT_HISTORY_MAX: no per-pixel budget */
#define HRT_REFINE_MAX_RADIUS 3u

typedef struct hrt_refine_rule { /* 32 bytes */
  uint32_t min_history;  /* >= 1: a pixel with fewer frames is always selected; a tap with fewer is skipped */
  uint32_t max_count;    /* >= min_history: a pixel with this many frames is never selected (its budget) */
  uint32_t radius;       /* 0..3: the criterion pools the (2 radius + 1)^2 window's pixels of the same surface */
  uint32_t flags;        /* must be 0 */
  float tolerance;       /* finite, > 0: the relative standard error of the mean a pixel is refined down to */
  float luminance_floor; /* finite, > 0: the pooled mean luminance is not taken below this */
  uint32_t reserved[2];  /* ignored */
} hrt_refine_rule;

typedef enum hrt_refine_method {
  HRT_REFINE_AUTO = 0,    /* FRAME: it measured faster on island at every share, on cave from 10 % on */
  HRT_REFINE_QUERIES = 1, /* the selected pixels as a compact list of radiance queries (hrt_radiance's kernels) */
  HRT_REFINE_FRAME = 2    /* hrt_trace of the whole frame, folded into the selected pixels only */
} hrt_refine_method;
#define HRT_REFINE_MOMENTS 1u /* hrt_refine / hrt_refine_until flags bit 0: fold the moments image M too */

typedef struct hrt_refine_stats { /* 48 bytes */
  uint32_t method_ran;       /* hrt_refine_method that ran (AUTO resolved; 0 when nothing was selected) */
  uint32_t query_method_ran; /* QUERIES: the hrt_query_method that ran, as hrt_radiance_stats; else 0 */
  uint64_t selected;         /* pixels whose bit is set in the mask */
  uint64_t scan_segments;    /* QUERIES: as hrt_radiance_stats; FRAME: 0 (the frame counts in hrt_stats) */
  uint64_t segments;
  uint64_t tri_tests;
  uint64_t reserved;         /* 0 */
} hrt_refine_stats;

/* What one hrt_refine_tiles pass ran. */
typedef struct hrt_refine_tiles_stats { /* 40 bytes */
  uint32_t kernel_ran;     /* hrt_kernel of the pass's launches; 0: nothing was selected, nothing ran */
  uint32_t whole_frame;    /* 1: the launches ran every tile (the fallback) */
  uint32_t tiles;          /* 8x8 tiles of the image */
  uint32_t tiles_selected; /* tiles with at least one selected real pixel */
  uint32_t items;          /* work items of the masked plan per frame (0 when whole_frame) */
  uint32_t reserved;       /* 0 */
  uint64_t selected;       /* pixels whose bit is set */
  uint64_t pixels_traced;  /* real pixels of the selected tiles (the image's pixels when whole_frame) */
} hrt_refine_tiles_stats;

/* The layouts every binding relies on (the Rust declarations in INTEGRATION.md are checked against
 * these by tests/test_rust_binding.py): std430 record sizes, the push block, and the host structs. */
#ifdef __cplusplus
#define HRT_STATIC_ASSERT(c, m) static_assert(c, m)
#else
#define HRT_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif
HRT_STATIC_ASSERT(sizeof(hrt_material) == 48, "std430 RayTracingMaterial");
HRT_STATIC_ASSERT(sizeof(hrt_ray) == 16, "std430 Ray");
HRT_STATIC_ASSERT(sizeof(hrt_sphere) == 64, "std430 Sphere");
HRT_STATIC_ASSERT(sizeof(hrt_triangle) == 64, "std430 Triangle");
HRT_STATIC_ASSERT(sizeof(hrt_mesh) == 80, "std430 Mesh");
HRT_STATIC_ASSERT(offsetof(hrt_mesh, len) == 28 && offsetof(hrt_mesh, material) == 32, "std430 Mesh layout");
HRT_STATIC_ASSERT(sizeof(hrt_push_constants) == 124, "push constant block (src/raytrace_pipeline.rs:125-139)");
HRT_STATIC_ASSERT(offsetof(hrt_push_constants, num_rays) == 80 && offsetof(hrt_push_constants, jitter_size) == 96 &&
                      offsetof(hrt_push_constants, height) == 120,
                  "push constant layout");
HRT_STATIC_ASSERT(sizeof(hrt_create_info) == 28 && offsetof(hrt_create_info, part_count) == 24, "hrt_create_info");
HRT_STATIC_ASSERT(sizeof(hrt_layout) == 28 && offsetof(hrt_layout, mode) == 24, "hrt_layout");
HRT_STATIC_ASSERT(sizeof(hrt_stats) == 64 && offsetof(hrt_stats, last_trace_ms) == 32 &&
                      offsetof(hrt_stats, wave_steps) == 40 && offsetof(hrt_stats, last_kernel) == 48 &&
                      offsetof(hrt_stats, last_frames) == 56,
                  "hrt_stats: 64 bytes since ABI 4");
HRT_STATIC_ASSERT(sizeof(hrt_present_info) == 24 && offsetof(hrt_present_info, pitch) == 16 &&
                      offsetof(hrt_present_info, flags) == 20,
                  "hrt_present_info");
HRT_STATIC_ASSERT(sizeof(hrt_fold_record) == 24 && offsetof(hrt_fold_record, max_delta) == 8 &&
                      offsetof(hrt_fold_record, abs_delta_sum) == 16,
                  "hrt_fold_record");
HRT_STATIC_ASSERT(sizeof(hrt_settle_rule) == 16 && offsetof(hrt_settle_rule, quiet_frames) == 8 &&
                      offsetof(hrt_settle_rule, flags) == 12,
                  "hrt_settle_rule");
HRT_STATIC_ASSERT(sizeof(hrt_ray_query) == 32 && offsetof(hrt_ray_query, t_max) == 12 &&
                      offsetof(hrt_ray_query, direction) == 16 && offsetof(hrt_ray_query, reserved) == 28,
                  "hrt_ray_query");
HRT_STATIC_ASSERT(sizeof(hrt_hit) == 32 && offsetof(hrt_hit, kind) == 4 && offsetof(hrt_hit, index) == 8 &&
                      offsetof(hrt_hit, mesh) == 12 && offsetof(hrt_hit, normal) == 16 && offsetof(hrt_hit, reserved) == 28,
                  "hrt_hit");
HRT_STATIC_ASSERT(sizeof(hrt_query_stats) == 24 && offsetof(hrt_query_stats, scan_rays) == 8 &&
                      offsetof(hrt_query_stats, tri_tests) == 16,
                  "hrt_query_stats");
HRT_STATIC_ASSERT(sizeof(hrt_occlusion_stats) == 32 && offsetof(hrt_occlusion_stats, reserved) == 4 &&
                      offsetof(hrt_occlusion_stats, scan_rays) == 8 && offsetof(hrt_occlusion_stats, tri_tests) == 16 &&
                      offsetof(hrt_occlusion_stats, occluded) == 24,
                  "hrt_occlusion_stats");
HRT_STATIC_ASSERT(sizeof(hrt_radiance_query) == 32 && offsetof(hrt_radiance_query, seed) == 12 &&
                      offsetof(hrt_radiance_query, centre) == 16 && offsetof(hrt_radiance_query, reserved) == 28,
                  "hrt_radiance_query");
HRT_STATIC_ASSERT(sizeof(hrt_radiance_stats) == 32 && offsetof(hrt_radiance_stats, reserved) == 4 &&
                      offsetof(hrt_radiance_stats, scan_segments) == 8 && offsetof(hrt_radiance_stats, segments) == 16 &&
                      offsetof(hrt_radiance_stats, tri_tests) == 24,
                  "hrt_radiance_stats");

HRT_STATIC_ASSERT(sizeof(hrt_denoise_info) == 32 && offsetof(hrt_denoise_info, method) == 8 &&
                      offsetof(hrt_denoise_info, sigma_colour) == 16 && offsetof(hrt_denoise_info, sigma_depth) == 24 &&
                      offsetof(hrt_denoise_info, reserved) == 28,
                  "hrt_denoise_info");

HRT_STATIC_ASSERT(sizeof(hrt_view) == 128 && offsetof(hrt_view, cam_alignment_mat) == 16 &&
                      offsetof(hrt_view, grid_first) == 80 && offsetof(hrt_view, grid_dx) == 96 &&
                      offsetof(hrt_view, grid_dy) == 112,
                  "hrt_view");
HRT_STATIC_ASSERT(sizeof(hrt_upsample_info) == 32 && offsetof(hrt_upsample_info, width) == 4 &&
                      offsetof(hrt_upsample_info, footprint) == 12 && offsetof(hrt_upsample_info, flags) == 16 &&
                      offsetof(hrt_upsample_info, sigma_normal) == 20 && offsetof(hrt_upsample_info, reserved) == 28,
                  "hrt_upsample_info");
HRT_STATIC_ASSERT(sizeof(hrt_resolve_info) == 32 && offsetof(hrt_resolve_info, offset_y) == 4 &&
                      offsetof(hrt_resolve_info, max_history) == 8 && offsetof(hrt_resolve_info, flags) == 12 &&
                      offsetof(hrt_resolve_info, reserved) == 16,
                  "hrt_resolve_info");
HRT_STATIC_ASSERT(sizeof(hrt_variance_info) == 32 && offsetof(hrt_variance_info, method) == 4 &&
                      offsetof(hrt_variance_info, min_history) == 12 && offsetof(hrt_variance_info, sigma_variance) == 16 &&
                      offsetof(hrt_variance_info, variance_floor) == 20 && offsetof(hrt_variance_info, sigma_depth) == 28,
                  "hrt_variance_info");
HRT_STATIC_ASSERT(sizeof(hrt_reproject_info) == 32 && offsetof(hrt_reproject_info, flags) == 4 &&
                      offsetof(hrt_reproject_info, depth_tolerance) == 8 &&
                      offsetof(hrt_reproject_info, min_normal_dot) == 12 && offsetof(hrt_reproject_info, reserved) == 16,
                  "hrt_reproject_info");
HRT_STATIC_ASSERT(sizeof(hrt_refine_rule) == 32 && offsetof(hrt_refine_rule, max_count) == 4 &&
                      offsetof(hrt_refine_rule, radius) == 8 && offsetof(hrt_refine_rule, flags) == 12 &&
                      offsetof(hrt_refine_rule, tolerance) == 16 && offsetof(hrt_refine_rule, luminance_floor) == 20 &&
                      offsetof(hrt_refine_rule, reserved) == 24,
                  "hrt_refine_rule");
HRT_STATIC_ASSERT(sizeof(hrt_refine_stats) == 48 && offsetof(hrt_refine_stats, query_method_ran) == 4 &&
                      offsetof(hrt_refine_stats, selected) == 8 && offsetof(hrt_refine_stats, scan_segments) == 16 &&
                      offsetof(hrt_refine_stats, segments) == 24 && offsetof(hrt_refine_stats, tri_tests) == 32 &&
                      offsetof(hrt_refine_stats, reserved) == 40,
                  "hrt_refine_stats");
HRT_STATIC_ASSERT(sizeof(hrt_refine_tiles_stats) == 40 && offsetof(hrt_refine_tiles_stats, whole_frame) == 4 &&
                      offsetof(hrt_refine_tiles_stats, tiles) == 8 && offsetof(hrt_refine_tiles_stats, tiles_selected) == 12 &&
                      offsetof(hrt_refine_tiles_stats, items) == 16 && offsetof(hrt_refine_tiles_stats, reserved) == 20 &&
                      offsetof(hrt_refine_tiles_stats, selected) == 24 && offsetof(hrt_refine_tiles_stats, pixels_traced) == 32,
                  "hrt_refine_tiles_stats");
HRT_STATIC_ASSERT(sizeof(hrt_motion) == 64 && offsetof(hrt_motion, flags) == 48 && offsetof(hrt_motion, reserved) == 52,
                  "hrt_motion");
HRT_STATIC_ASSERT(sizeof(hrt_motion_tables) == 32 && offsetof(hrt_motion_tables, n_spheres) == 8 &&
                      offsetof(hrt_motion_tables, meshes) == 16 && offsetof(hrt_motion_tables, n_meshes) == 24,
                  "hrt_motion_tables");
HRT_STATIC_ASSERT(sizeof(hrt_first_hits_stats) == 48 && offsetof(hrt_first_hits_stats, reserved) == 4 &&
                      offsetof(hrt_first_hits_stats, tiles) == 8 && offsetof(hrt_first_hits_stats, tiles_listed) == 12 &&
                      offsetof(hrt_first_hits_stats, tiles_empty) == 16 &&
                      offsetof(hrt_first_hits_stats, tiles_fallback) == 20 &&
                      offsetof(hrt_first_hits_stats, scan_rays) == 24 && offsetof(hrt_first_hits_stats, tri_tests) == 32 &&
                      offsetof(hrt_first_hits_stats, entries_tested) == 40,
                  "hrt_first_hits_stats");

typedef struct hrt_context hrt_context;

/* Trace kernel variants (HRT_OPT_KERNEL_VARIANT).  All produce byte-identical frames and counters;
 * they differ only in how much of the reference's brute-force work they prove unnecessary. */
typedef enum hrt_kernel {
  HRT_KERNEL_AUTO = 0,        /* BUNDLE below 256 mesh triangles; then, with a useful hierarchy
                                 (HRT_SCENE_BVH_SAH_MILLI <= 100), BUNDLE_WQ while it fits LDS; else
                                 BUNDLE_CULL_LDS while the triangle buffer fits LDS (else BUNDLE_CULL)
                                 below 4096 triangles (any count for a poor hierarchy); BUNDLE_BVH above */
  HRT_KERNEL_LITERAL = 1,     /* raytracing.glsl's loop shape, the full test on every triangle */
  HRT_KERNEL_BRUTE = 2,       /* fused sample/bounce loop, two-stage exact pre-test, triangles via SGPRs */
  HRT_KERNEL_BRUTE_LDS = 3,   /* BRUTE with the scene resident in LDS (falls back to BRUTE above 160 KiB) */
  HRT_KERNEL_BUNDLE = 4,      /* primary rays: lane-parallel bundle cull; bounces: deferred, BRUTE test */
  HRT_KERNEL_BUNDLE_CULL = 5, /* BUNDLE + lane-parallel origin-box / direction-cone cull of bounce rays */
  HRT_KERNEL_BUNDLE_BVH = 6,  /* BUNDLE + per-lane BVH traversal of bounce rays (hierarchy built by
                                 hrt_set_scene; falls back to BUNDLE_CULL above 64 meshes or 2^18
                                 mesh triangles) */
  HRT_KERNEL_BUNDLE_CULL_LDS = 7, /* BUNDLE_CULL with the triangle buffer resident in LDS (512/1024-thread
                                    workgroups; falls back to BUNDLE_CULL above ~3,300 triangles) */
  HRT_KERNEL_BUNDLE_BVH_LDS = 8,  /* BUNDLE_BVH with the hierarchy and triangles in LDS (1024-thread
                                    workgroups; falls back to BUNDLE_BVH when they exceed 160 KiB) */
  HRT_KERNEL_BUNDLE_WQ = 9,       /* bounce segments through the hierarchy as (ray, node) / (ray, triangle)
                                    pairs on per-wave LDS stacks, 64 pairs per step (1024-thread
                                    persistent workgroups, nodes in LDS; falls back to BUNDLE_BVH_LDS when
                                    they do not fit or leaves exceed 4 triangles) */
  HRT_KERNEL_BUNDLE_WQ_L2 = 10,   /* BUNDLE_WQ for hierarchies that do not fit the LDS: the same pair traversal
                                    with the node image (breadth first, up to 65,535 nodes = 3 MB) read from
                                    global memory / L2 and only the top of the tree (HRT_OPT_WQ_LDS_NODES)
                                    in the LDS the pair stacks leave free; no sky lane.  Runs when the image
                                    exists (fewer than 65,536 nodes, leaves of at most 4 triangles, at most
                                    64 meshes) and the stacks fit; else falls back as BUNDLE_WQ does.
                                    HRT_KERNEL_AUTO does not pick it yet: scenes past BUNDLE_WQ's limit keep
                                    BUNDLE_BVH.  A later change of AUTO will rest on the measurements of
                                    DESIGN.md 22 (profiles/wq_l2_ab.txt; 1080p, 64 spp, 8 bounces, ms per
                                    frame against BUNDLE_BVH): island@2 2.73 against 20.75, cave@2 9.93
                                    against 219.96, island@4 9.57 against 52.70, island@8 98.5 against 229.9
                                    (bound by its band lists; at 320x180 no win is established there).  A
                                    scene that fits BUNDLE_WQ runs 14% slower on this variant. */
} hrt_kernel;

/* Option keys for hrt_set_option. */
typedef enum hrt_option {
  /* trace kernel variant (hrt_kernel), default HRT_KERNEL_AUTO */
  HRT_OPT_KERNEL_VARIANT = 1,
  /* 1 = count segments / triangle tests on the device (default); 0 = off; 2 = also the bundle
   * kernels' cull diagnostics (hrt_get_diagnostics) */
  HRT_OPT_COUNTERS = 2,
  /* bundle kernel: a wave runs its bounce (non-primary) segments once this many lanes wait for one,
   * or when no lane has a primary segment left (1..64; default 0 = auto: 28 for BUNDLE_WQ (36 with per-node radii), else 48;
   * results do not depend on it) */
  HRT_OPT_SECONDARY_BATCH = 3,
  /* BUNDLE_BVH / BUNDLE_WQ: triangles per leaf of the hierarchy the next hrt_set_scene builds (1..16;
   * default 0 = auto: 2 up to 8192 mesh triangles, else 4) */
  HRT_OPT_BVH_LEAF_SIZE = 4,
  /* persistent kernels: a heavy tile (HRT_OPT_SPLIT_FACTOR) of the previous trace runs as this many
   * work items of 8/k rows each, scheduled first: at most this many (1 = off, 2, 4, 8; default 0 =
   * auto: BUNDLE_WQ 8, the others 1), 2 / 4 / 8 as the tile's cost passes 1 / 2 / 4 x the heavy
   * threshold.  The frame's time is set by its slowest tiles' sample chains; results do not depend on it. */
  HRT_OPT_SPLIT = 5,
  /* heavy tile: its cost in the previous trace exceeds this multiple of a resident wave's fair share
   * (sum of tile costs / resident waves), to an eighth octave (0: every tile is heavy; default -1 =
   * auto: BUNDLE_WQ 1.25 in a launch of several frames (hrt_compute_n), else 2 (3 when a resident
   * wave gets at most 6 tiles); the others 3 when there are more than 4 tiles per resident wave, else 1) */
  HRT_OPT_SPLIT_FACTOR = 6,
  /* persistent kernels: heavy tiles (as above) run at raised wave issue priority (1 default, 0 off;
   * libhip_raytrace_debug.so only: 2 = a planned trace runs ONLY the heavy tiles, the frame is
   * incomplete -- a diagnostics mode the production library rejects) */
  HRT_OPT_PRIORITY = 7,
  /* libhip_raytrace_debug.so only (latency experiments): persistent kernels launch workgroups for at
   * most this many CUs (0 = all).  The production library rejects the key. */
  HRT_OPT_GRID_CUS = 8,
  /* BUNDLE_CULL_LDS with HRT_OPT_SPLIT = 1: heavy tiles run cooperatively, every wave of a workgroup
   * on the same tile with the bounce cull's chunks dealt out over the waves (1 default, 0 off) */
  HRT_OPT_COOP = 9,
  /* BUNDLE_WQ: per-wave node-pair stack capacity (0 = what fits the LDS, default; else at most that,
   * rounded down to a multiple of 64, >= 128).  A step that could overflow it walks its pairs'
   * subtrees stacklessly instead; results do not depend on it (tests force the fallback with 128). */
  HRT_OPT_WQ_NODE_CAP = 10,
  /* persistent kernels: the first trace of a context (no previous tile costs) is preceded by a
   * 1-sample probe trace into a scratch image whose per-tile costs plan it (1 default, 0 off).
   * Frames, counters and the trace timing are unaffected. */
  HRT_OPT_PROBE = 11,
  /* hrt_compute_n: frames traced by one persistent launch (default 64, 1 = one launch per frame;
   * also capped at 1 GiB of frame images).  Results do not depend on it. */
  HRT_OPT_FRAMES_PER_LAUNCH = 12,
  /* hrt_trace: consecutive traces rotate over this many trace lanes (own stream + trace image) so that
   * the next frame's trace starts while the current one finishes (default 3; 0 or 1 = one lane, each
   * trace after the previous frame's combiner).  Results do not depend on it.  Diagnostics
   * (HRT_OPT_COUNTERS = 2) use one lane. */
  HRT_OPT_OVERLAP = 13,
  /* hrt_trace: a trace issued while another lane's trace still runs launches its persistent grid over
   * 1/value of the CUs (default 2; 1 = always every CU), so consecutive frames share the chip; a trace
   * issued to an idle GPU always gets every CU.  Results do not depend on it. */
  HRT_OPT_BUSY_SPLIT = 14,
  /* BUNDLE_WQ: children tested per node visit in the hierarchy the next hrt_set_scene builds (2 = the
   * binary tree, 3 or 4 = groups of up to that many collapsed from it; default 4).  Results do not
   * depend on it. */
  HRT_OPT_BVH_WIDTH = 15,
  /* BUNDLE_WQ: the radius R in a node's box margin a + b R (DESIGN.md "BVH cull": R bounds the ray
   * origin's distance to every vertex below the node).  1 = the origin's distance to the farthest
   * scene-box corner (once per ray); 2 = to the farthest corner of the node's own box (per node: more
   * arithmetic, tighter boxes where margins are wide); default 0 = auto: 2 when
   * HRT_SCENE_BVH_MARGIN_MILLI > 100 (cave), else 1.  Results do not depend on it. */
  HRT_OPT_WQ_NODE_RADIUS = 16,
  /* hrt_comm_init / collective hrt_read_image: milliseconds a rank waits for its peers in the status
   * agreement or the gather before it aborts the communicator (ncclCommAbort) and returns
   * HRT_ERR_COMM (default 120000; 0 = wait forever).  Per context. */
  HRT_OPT_COMM_TIMEOUT_MS = 17,
  /* hrt_trace + hrt_accumulate (the realtime loop): 1 = the combine of a traced frame is deferred --
   * the trace writes a slot of a ring of up to 16 frame images (allocated by the first trace, at most
   * 512 MiB) and the recorded frames are folded into the accumulator in frame order at the next
   * hrt_read_image / hrt_synchronize / hrt_stream / hrt_compute_n or when the ring is full, so no
   * combiner kernel waits between two traces; 0 (default) = one combiner dispatch per hrt_accumulate.
   * The bytes are the same either way.  Measured on island 1080p (r03b): 2.81-2.86 ms per frame
   * deferred against 2.53 immediate -- without the combiners pacing them, the three lanes' persistent
   * traces all run at once and contend for the CUs -- so it is off by default. */
  HRT_OPT_DEFER_COMBINE = 18,
  /* 1 = every fold on the context (hrt_accumulate, hrt_accumulate_present -- which then runs as its two
   * passes, same bytes --, each frame of hrt_compute_n's multi-frame fold, each frame of a deferred-combine
   * flush) appends one hrt_fold_record to the context's ring, in fold order, computed on the device by the
   * combiner itself; 0 (default) = off: every path issues the kernels it issues without this option.
   * Setting it (to 0 or 1) empties the ring and zeroes the total.  Accumulator, trace image, targets and
   * hrt_stats are byte for byte the same either way.  On an hrt_comm_init_all group each member records
   * its own rows when its own option is set; there is no collective. */
  HRT_OPT_FOLD_RECORDS = 19,
  /* BUNDLE_WQ: the sky lane.  1 = a planned launch's sky items (whole tiles whose primary list is empty, in
   * a scene without spheres) run on a lean kernel of their own (trace_sky), resident beside the main
   * kernel's workgroups as one more wave per SIMD and fed from the far end of the same work queue; 0 = every
   * item on the main kernel; default -1 = auto: on where it was measured faster -- launches of at least 128
   * work units (tile x frame) per resident wave at 64 or more samples per pixel: hrt_compute_n /
   * hrt_compute_until launches of a whole 1080p frame from 17 frames up (island and cave) -- and off
   * everywhere else, where it was measured slower (shorter launches, the per-frame loop, row-tile parts of
   * 2 and 8, island 4K at 16 spp) or not measured at all (other sample counts and sizes): off is the
   * code path without the lane, so auto never costs more than 0.  Diagnostics (HRT_OPT_COUNTERS = 2), probes and
   * timeline builds always keep every item on the main kernel.  Results do not depend on it. */
  HRT_OPT_SKY_LANE = 20,
  /* BUNDLE_WQ_L2: nodes of the breadth-first image (the top of the tree) kept in LDS.  -1 (default) = auto:
   * the pair stacks get their BUNDLE_WQ capacities first (1,024 node pairs, or the HRT_OPT_WQ_NODE_CAP
   * request) and the nodes what is left of the 160 KiB (about 1,100 at leaves of 4); 0 = none, every node
   * is read from global memory; n = min(n, the image's nodes, what fits beside node stacks of 128 pairs),
   * the node stacks then taking what is left.  Results do not depend on it; the other kernels ignore it. */
  HRT_OPT_WQ_LDS_NODES = 21,
  /* bundle kernels' fused loop: an iteration that runs a bounce batch (HRT_OPT_SECONDARY_BATCH) runs the
   * ready lanes' primary segments too only once this many lanes are ready for one; an iteration without a
   * batch runs them whenever a lane is ready.  A lane held back starts its sample with the iteration that
   * runs it.  1..64 (1 = in every iteration with a ready lane); default 0 = auto: 48 for BUNDLE_WQ, else 1
   * (hrt_launch_plan.h, DESIGN.md 29: BUNDLE_WQ measured faster still at 40 with HRT_OPT_SECONDARY_BATCH 36, 44 with per-node radii).  Results do not depend on it. */
  HRT_OPT_PRIMARY_BATCH = 22,
  /* libhip_raytrace_debug.so only (tests): the value-th device allocation of the next hrt_set_scene
   * fails with HRT_ERR_OUT_OF_MEMORY (0 = off) */
  HRT_DEBUG_OPT_FAIL_ALLOC = 1001,
  /* libhip_raytrace_debug.so only (tests): BUNDLE_WQ's per-wave triangle-pair stack holds at most this
   * many pairs (0 = what fits; else >= 128, rounded down to a multiple of 64): bursts of kept leaves
   * beyond it are tested in place, the path the tests force with 128.  Results do not depend on it. */
  HRT_DEBUG_OPT_WQ_TRI_CAP = 1002,
  /* libhip_raytrace_debug.so only (tests): 1 = the persistent kernels' waves always take their work
   * items 4 at a time, so a multi-frame launch runs frame runs (an item's consecutive frames in one
   * pass, hrt_kernels.hip trace_fused_split) at any image size -- the full frames take them only while
   * many items remain.  Results do not depend on it. */
  HRT_DEBUG_OPT_GRAB_RUNS = 1003,
  /* builds with -DHRT_TIMELINE=1 only (tuning, tools/timeline.py): record, for each work item the persistent
   * kernels execute, its start / end time (s_memrealtime, 100 MHz), item word, frame, run length and
   * resident wave -- up to value records per launch (hrt_debug_timeline).  Other builds reject the key. */
  HRT_DEBUG_OPT_TIMELINE = 1004,
  /* libhip_raytrace_debug.so only (tests): an hrt_compute_n frame-image allocation of more than value
   * bytes fails as if the device were out of memory (0 = off), so the fallback from a whole launch's
   * images to the call's own frames runs.  Results do not depend on it. */
  HRT_DEBUG_OPT_STACK_LIMIT = 1005
} hrt_option;

/* Cull diagnostics of the bundle kernels (HRT_OPT_COUNTERS = 2), summed since the last reset. */
typedef enum hrt_diag {
  HRT_DIAG_PRIMARY_ITERS = 0,      /* wave iterations that ran the primary bundle path (HRT_OPT_PRIMARY_BATCH) */
  HRT_DIAG_PRIMARY_CONSIDERED = 1, /* camera-facing triangles bounded (per wave) */
  HRT_DIAG_PRIMARY_SURVIVORS = 2,  /* ... of which survived the bundle cull */
  HRT_DIAG_BOUNCE_ITERS = 3,       /* wave iterations that ran a bounce batch */
  HRT_DIAG_BOUNCE_CONSIDERED = 4,  /* triangles bounded by the bounce pre-cull (per wave) */
  HRT_DIAG_BOUNCE_SURVIVORS = 5,   /* ... of which survived */
  HRT_DIAG_BOUNCE_LANES = 6,       /* lanes in bounce batches */
  HRT_DIAG_BVH_VISITS = 7,         /* BUNDLE_BVH: node visits summed over bounce lanes */
  HRT_DIAG_BVH_PRIM_TESTS = 8,     /* BUNDLE_BVH: leaf triangles reached, summed over bounce lanes */
  HRT_DIAG_BVH_BAND_TESTS = 9,     /* BUNDLE_BVH: grazing-band triangles tested, summed over bounce lanes */
  HRT_DIAG_PRIMARY_CYCLES = 10,    /* shader clocks per wave in the primary cull + tests, summed */
  HRT_DIAG_BOUNCE_CYCLES = 11,     /* ... in the bounce-batch path */
  HRT_DIAG_SHADE_CYCLES = 12,      /* ... in shading (scatter, RNG, colour) */
  HRT_DIAG_BOUNCE_STAGE2 = 13,     /* BUNDLE_CULL: bounce survivors with some lane's num_t > 0 */
  HRT_DIAG_BOUNCE_FRONT = 14,      /* ... and some such lane front-facing (dn < 0) */
  HRT_DIAG_BVH_TRIPS = 15,         /* BUNDLE_BVH: traversal loop iterations per bounce batch (wave), summed */
  HRT_DIAG_BVH_LEAF_TRIPS = 16,    /* ... of which some lane tested a leaf */
  HRT_DIAG_BAND_SCAN_MAX = 17,     /* BUNDLE_WQ: grazing-band entries of the longest list per bounce batch, summed */
  HRT_DIAG_BAND_SCAN_LEN = 18,     /* ... of every bounce lane's list, summed */
  HRT_DIAG_SKY_ITEMS = 19,         /* work items (waves) whose primary list is empty: every segment a miss */
  HRT_DIAG_SKY_CYCLES = 20,        /* ... their shader clocks per wave, summed */
  HRT_DIAG_PRIMARY_LANES = 21,     /* fused loop: primary lanes of the iterations that ran the primary path
                                      (each starts its sample there: one per primary segment, whatever the thresholds) */
  HRT_DIAG_LOOP_ITERS = 22,        /* fused-loop iterations (waves) with a lane not yet done: each ran a phase */
  HRT_DIAG_LIVE_LANES = 23,        /* ... and their lanes not yet done, summed */
  HRT_DIAG_WQ_STEPS_16 = 24,       /* BUNDLE_WQ: pair steps with 1-16 node pairs (waves) */
  HRT_DIAG_WQ_STEPS_32 = 25,       /* ... 17-32 */
  HRT_DIAG_WQ_STEPS_48 = 26,       /* ... 33-48 */
  HRT_DIAG_WQ_STEPS_64 = 27,       /* ... 49-64 */
  HRT_DIAG_WQ_MEMBERS = 28,        /* ... valid members of the popped node groups, summed (vs 4 slots each) */
  HRT_DIAG_DIR_LANES = 29,         /* bounce-batch lanes whose direction the batch computed (two-phase shading) */
  HRT_DIAG_PRIMARY_DEFERRED = 30,  /* fused loop: ready lanes of the iterations that ran a bounce batch without the primary path */
  HRT_DIAG_BATCH_ONLY_ITERS = 31,  /* ... those iterations */
  HRT_NUM_DIAG = 32
} hrt_diag;

/* What hrt_set_scene built for BUNDLE_BVH (hrt_get_scene_info). */
typedef enum hrt_scene_info {
  HRT_SCENE_BVH_NODES = 0,      /* hierarchy nodes */
  HRT_SCENE_BVH_PRIMS = 1,      /* (mesh, triangle) entries in its leaves */
  HRT_SCENE_BVH_IRREGULAR = 2,  /* entries outside the cull analysis (non-finite, normal != e1 x e2, ...):
                                   tested against every bounce ray */
  HRT_SCENE_BVH_NEVER = 3,      /* entries with a zero normal, which the reference never accepts */
  HRT_SCENE_BVH_BUILT = 4,      /* 1 if built (0: > 64 meshes or > 2^18 entries -> BUNDLE_BVH runs BUNDLE_CULL) */
  HRT_SCENE_BVH_BAND_ENTRIES = 5, /* grazing-band list entries over all direction cells */
  HRT_SCENE_BVH_SAH_MILLI = 6,  /* 1000 x the expected leaf triangle tests of a uniform random ray per
                                   entry (surface-area estimate): < ~30 for a useful hierarchy; large
                                   overlapping triangles (a soup) give ~500, and auto then culls instead */
  HRT_SCENE_BVH_MARGIN_MILLI = 7, /* 1000 x the mean over nodes of the box margin at R = the scene box's
                                     diagonal / the box's largest extent (island 26, cave 197) */
  HRT_NUM_SCENE_INFO = 8
} hrt_scene_info;

uint32_t hrt_abi_version(void);
/* Identity of the device code (hash of the kernel sources and build flags): measurement records
 * (profiles/pmc_traffic.json) carry it, so counters of an older kernel are never applied to this one. */
const char* hrt_build_id(void);
/* 1 for libhip_raytrace_debug.so (accepts the debug-only options above), 0 for the production library. */
uint32_t hrt_debug_build(void);
/* libhip_raytrace_debug.so: every device buffer of the context is surrounded by 4 KiB guard bands of a
 * fixed pattern; this synchronizes and counts the buffers and those whose bands were overwritten (a
 * kernel wrote outside its buffer).  The production library returns HRT_ERR_INVALID_ARGUMENT. */
hrt_status hrt_debug_check_guards(hrt_context* ctx, uint32_t* buffers, uint32_t* corrupted);

hrt_status hrt_create(const hrt_create_info* info, hrt_context** out_ctx);
void hrt_destroy(hrt_context* ctx);

/* Upload the scene.  rays: n_rays == width*height records indexed by global pixel id x + y*W
 * (or NULL / 0 to keep the rays of an earlier hrt_generate_rays / hrt_set_scene).
 * spheres/tris/meshes may be NULL when their count is 0 (the reference's "null object" records are
 * not needed).  Every mesh range must lie inside [0, n_tri).  Copies before returning. */
hrt_status hrt_set_scene(hrt_context* ctx, const hrt_ray* rays, uint32_t n_rays, const hrt_sphere* spheres,
                         uint32_t n_spheres, const hrt_triangle* tris, uint32_t n_tris, const hrt_mesh* meshes,
                         uint32_t n_meshes);

/* One dispatch of raytracing.glsl (or its init clear when pc->init != 0).  pc->width/height must
 * equal the context's; pc->num_spheres/num_meshes must not exceed the uploaded counts. */
hrt_status hrt_trace(hrt_context* ctx, const hrt_push_constants* pc);

/* One dispatch of image_combiner.glsl with next_image = this context's trace image.  Any uint32_t frame
 * is folded as the shader's arithmetic folds it: frame 0 clears, and at frame 0xFFFFFFFF, whose frame + 1
 * wraps to 0, the division is IEEE's division by zero (a channel with a nonzero numerator becomes 255,
 * 0 / 0 becomes 0). */
hrt_status hrt_accumulate(hrt_context* ctx, uint32_t frame);

/* The frame loop of compute_n_then_render (src/raytracing_app.rs:198-227, without the present):
 * for k = pc->rng_offset .. pc->rng_offset + n - 1, one trace of pc with rng_offset = k followed by
 * hrt_accumulate(ctx, k) -- byte for byte the result of that loop of hrt_trace / hrt_accumulate
 * calls, the trace image holding the last frame afterwards.  The persistent kernels trace up to
 * HRT_OPT_FRAMES_PER_LAUNCH frames in one launch (each frame its own image), so that the long
 * per-pixel sample chains of one frame run beside the other frames' work instead of ending each
 * frame alone; the combiner then folds the frames in order.  pc->init must be 0. */
hrt_status hrt_compute_n(hrt_context* ctx, const hrt_push_constants* pc, uint32_t n);

/* Closest hit of caller rays: hits[i] = the reference's world_hit (raytracing.glsl:267-288) of rays[i] against
 * the uploaded scene (all its spheres and meshes), by DESIGN.md §2 S11: the direction normalised by S4, the
 * running closest started at min(t_max, FLT_MAX), spheres first, then meshes in buffer order behind the
 * reference's AABB test, a hit accepted iff dist > 0.001 and dist < the running closest.  Every method gives
 * the same bytes.  BLOCKING; ordered on the context's stream after the work issued so far; touches no trace
 * lane, image, hrt_stats, fold record or ticket.  rays / hits: host memory (staged in chunks) or memory of
 * the context's device (then 16-byte aligned), each decided by hipPointerGetAttributes.  stats may be NULL.
 * n == 0: OK, nothing done.  HRT_ERR_INVALID_ARGUMENT (unknown method, NULL rays / hits with n > 0, a
 * misaligned device pointer) and HRT_ERR_NO_SCENE are decided before anything is enqueued. */
hrt_status hrt_intersect(hrt_context* ctx, const hrt_ray_query* rays, uint32_t n, uint32_t method, hrt_hit* hits,
                         hrt_query_stats* stats);

/* The same for the un-jittered primary rays of the pixels [x0, x0 + w) x [y0, y0 + h) (global pixel
 * coordinates of pc's camera; trace-image rows: the present pass flips them): origin pc->cam_pos, direction
 * normalize(mat3(pc->cam_alignment_mat) c) with c the context's ray centre of pixel x + y W (the row-wise
 * product of get_ray_dir, zero jitter, no RNG draw), t_max = FLT_MAX, pc's sphere and mesh counts (validated
 * as hrt_trace validates them).  hits receives w h records, row-major.  Works on any context (a row-tile part
 * holds every ray centre); not a collective.  An empty rectangle: OK, nothing done; one outside the image:
 * HRT_ERR_INVALID_ARGUMENT. */
hrt_status hrt_intersect_primary(hrt_context* ctx, const hrt_push_constants* pc, uint32_t x0, uint32_t y0,
                                 uint32_t w, uint32_t h, uint32_t method, hrt_hit* hits, hrt_query_stats* stats);

/* Any hit of caller rays, one bit per ray: ray i is occluded iff hrt_intersect on the same
 * context, ray and method returns kind != 0 -- a sphere or triangle exists that world_hit accepts with
 * 0.001 < dist < min(t_max, FLT_MAX), behind the meshes' AABB test.  Ray i is bit i & 31 of word i >> 5; the call
 * writes exactly ceil(n / 32) words, each in full, the unused high bits of the last one 0, and nothing beyond
 * them.  Methods, fallbacks and AUTO as hrt_intersect; every method gives the same bits.  The traversals stop
 * a ray at its first accepted hit and start its running closest at min(t_max, FLT_MAX), so a short segment
 * walks only the hierarchy near it.  BLOCKING; ordered on the context's stream after the work issued so far;
 * touches no trace lane, image, hrt_stats, fold record or ticket.  rays: host memory (staged in chunks) or
 * memory of the context's device (then 16-byte aligned); bits: host memory or memory of the context's device
 * (then 4-byte aligned).  stats may be NULL.  n == 0: OK, nothing written.  HRT_ERR_INVALID_ARGUMENT (unknown
 * method, NULL rays / bits with n > 0, a misaligned device pointer) and HRT_ERR_NO_SCENE are decided before
 * anything is enqueued. */
hrt_status hrt_occluded(hrt_context* ctx, const hrt_ray_query* rays, uint32_t n, uint32_t method, uint32_t* bits,
                        hrt_occlusion_stats* stats);

/* The path tracer for caller-chosen samples: query i is the reference's main() for a virtual
 * pixel, and rgba[4 i .. 4 i + 3] is exactly what main() stores into an RGBA32F image:
 *     state = seed; colour = 0
 *     for s in 0 .. num_samples - 1:
 *         dir = get_ray_dir(pc, centre, state)               -- three draws always; pc's matrix and jitter_size
 *         colour += trace_ray(origin, normalize(dir), state)  -- the second normalize, as main() applies it
 *     out = (colour / float(num_samples), 1.0)
 * Of pc the call uses cam_alignment_mat, jitter_size, num_samples, max_bounces, use_environment_light, and
 * num_spheres / num_meshes (validated against the uploaded counts as hrt_trace validates them); it ignores
 * cam_pos, rng_offset, num_rays, width and height; pc->init must be 0.  Consequences:
 *   - the query (cam_pos, rng_offset * 719393 + id, ray centre id) under a frame's own push block is that
 *     frame's pixel id, bit for bit (the seed map is a bijection on uint32: 719393 is odd);
 *   - a fixed direction d is an identity matrix with jitter 0 and centre = d; it still burns the three draws
 *     and is normalised twice;
 *   - num_samples <= 0 gives colour / float(num_samples) of a zero colour as the frame kernels store it: 0/0 =
 *     NaN in rgb at 0 (-0 below it);
 *   - max_bounces < 0 gives 0.
 * Every segment takes S11's regularity test (hrt_radiance_stats.scan_segments); an irregular one is answered
 * by the literal scan whatever the method.  Methods and fallbacks as hrt_intersect, and every method gives the
 * same bytes and the same three counts; HRT_QUERY_AUTO here is PAIRS when it fits, else BVH, else SCAN --
 * unlike hrt_intersect's, on purpose: every segment after a query's first is a bounce ray.
 * BLOCKING; ordered on the context's stream after the work issued so far; touches no trace lane, image,
 * hrt_stats, counter, fold record or ticket; works on any context (a row-tile part too) and is no collective.
 * queries, rgba: host memory (staged in chunks of 65,536) or memory of the context's device (then 16-byte
 * aligned).  stats may be NULL.  n == 0: OK, nothing written.  HRT_ERR_INVALID_ARGUMENT (unknown method,
 * pc->init, counts beyond the scene, NULL queries / rgba with n > 0, a misaligned device pointer) and
 * HRT_ERR_NO_SCENE are decided before anything is enqueued. */
hrt_status hrt_radiance(hrt_context* ctx, const hrt_push_constants* pc, const hrt_radiance_query* queries, uint32_t n,
                        uint32_t method, float* rgba /* n x 4 */, hrt_radiance_stats* stats);

/* The records of the newest min(cap, available) folds (HRT_OPT_FOLD_RECORDS = 1), oldest first; the ring
 * keeps the last HRT_FOLD_RECORD_RING.  Folds deferred combines and synchronizes the context, as
 * hrt_get_stats does.  *count = the records copied; *total (may be NULL) = the records appended since the
 * option was last set.  out may be NULL when cap is 0. */
hrt_status hrt_get_fold_records(hrt_context* ctx, hrt_fold_record* out, uint32_t cap, uint32_t* count,
                                uint64_t* total);

/* hrt_compute_n, stopped after the first run of quiet frames.  Let r_1, r_2, ... be the fold records of the
 * frames pc->rng_offset, pc->rng_offset + 1, ... as hrt_compute_n would fold them, and m the smallest index
 * >= rule->quiet_frames such that r_(m - quiet_frames + 1) ... r_m are all quiet (hrt_settle_rule).  If
 * m <= max_frames: *frames_done = m, *settled = 1; else *frames_done = max_frames, *settled = 0 (settled may
 * be NULL).  On return the accumulator, the trace image and hrt_stats.accumulates are byte for byte those of
 * hrt_compute_n(ctx, pc, *frames_done); with HRT_OPT_FOLD_RECORDS = 1 the ring gains exactly *frames_done
 * records (the call works with the option off too).  max_frames == 0: OK, 0 frames, not settled.
 * BLOCKING: the counts are needed on the host, so the call waits for each launch's count pass (a launch
 * holds min(HRT_OPT_FRAMES_PER_LAUNCH, frames left) frames on the persistent kernels, else one frame).
 * hrt_stats.traces, segments and tri_tests count every frame TRACED: the frames of the last launch past
 * the stop are traced and discarded, so they exceed hrt_compute_n(*frames_done)'s by up to one launch;
 * bound the waste with HRT_OPT_FRAMES_PER_LAUNCH.
 * HRT_ERR_INVALID_ARGUMENT before anything is enqueued (the message names the reason): a NULL rule or
 * frames_done, rule->flags != 0, rule->quiet_frames == 0, pc->init != 0, a context of a row-tile partition
 * (part_count > 1) and a context joined to any communicator (the parts would stop at different frames). */
hrt_status hrt_compute_until(hrt_context* ctx, const hrt_push_constants* pc, uint32_t max_frames,
                             const hrt_settle_rule* rule, uint32_t* frames_done, uint32_t* settled);

/* Copy an image (row-major, x 4 channels) into dst, host or device memory.  Blocking.
 *  - Without a communicator, or with image_id | HRT_IMG_LOCAL: this context's local rows
 *    (local_rows x width); bytes >= that in fmt.
 *  - With one (hrt_comm_init / hrt_comm_init_all): the FULL frame (height x width), gathered from every
 *    part with one ncclGather to rank 0 and un-interleaved on rank 0's device.  hrt_comm_init: a
 *    collective -- every rank calls it; dst / bytes are used on rank 0 only (may be NULL elsewhere).
 *    Every rank first agrees on the call's status: if any rank's arguments or local image are bad,
 *    every rank returns an error (HRT_ERR_COMM on the others) and none enters the gather; a peer that
 *    does not arrive within HRT_OPT_COMM_TIMEOUT_MS aborts the communicator (later calls: HRT_ERR_COMM).
 *    hrt_comm_init_all: any context of the group may call it alone; the frame lands in dst. */
hrt_status hrt_read_image(hrt_context* ctx, uint32_t image_id, uint32_t fmt, void* dst, size_t bytes);

/* Checkpoint / resume (new): overwrite this context's local rows of the accumulated
 * image with bytes an earlier hrt_read_image(HRT_IMG_ACCUM, fmt) returned, in the context's own format
 * (HRT_FMT_RGBA8 for HRT_MODE_RGBA8, HRT_FMT_RGBA32F for HRT_MODE_RGBA32F; bytes = local_rows * width
 * * 4 or 16).  Continuing with frame numbers from the saved count reproduces an uninterrupted render
 * byte for byte.  src may be host or device memory. */
hrt_status hrt_load_accumulator(hrt_context* ctx, uint32_t fmt, const void* src, size_t bytes);

/* ---- multi-GPU framebuffer gather (RCCL is loaded on first use) ------------------- */
#define HRT_COMM_ID_BYTES 128 /* == sizeof(ncclUniqueId) */
typedef enum hrt_comm_transport {
  HRT_COMM_NONE = 0,        /* no communicator */
  HRT_COMM_RCCL = 1,        /* hrt_comm_init: one process / thread per GPU, ncclCommInitRank */
  HRT_COMM_RCCL_GROUP = 2,  /* hrt_comm_init_all on distinct devices: ncclCommInitAll, grouped ncclGather */
  HRT_COMM_DEVICE_COPY = 3  /* hrt_comm_init_all with contexts sharing a device: device-to-device copies */
} hrt_comm_transport;
/* A fresh RCCL unique id (ncclGetUniqueId) for hrt_comm_init; rank 0 creates it and shares the bytes. */
hrt_status hrt_comm_unique_id(uint8_t id[HRT_COMM_ID_BYTES]);
/* Joins ctx -- part `rank` of a `world`-way row-tile partition (hrt_create_info), or the whole image
 * when world == 1 -- to the communicator named by id.  Collective: blocks until all ranks joined.
 * The root's buffers are allocated before the communicator is created, and the ranks agree on the
 * outcome: a rank whose partition does not match or whose allocation failed makes every rank return
 * an error with no communicator (a NULL id, rank >= world or a missing RCCL cannot join at all). */
hrt_status hrt_comm_init(hrt_context* ctx, const uint8_t id[HRT_COMM_ID_BYTES], uint32_t rank, uint32_t world);
/* One process driving every part: ctxs[i] must be part i of n (same size, mode, row tile). */
hrt_status hrt_comm_init_all(hrt_context* const* ctxs, uint32_t n);
/* rank / world / hrt_comm_transport of ctx's communicator (0 / 1 / HRT_COMM_NONE without one). */
hrt_status hrt_comm_info(const hrt_context* ctx, uint32_t* rank, uint32_t* world, uint32_t* transport);

hrt_status hrt_get_layout(const hrt_context* ctx, hrt_layout* out);
hrt_status hrt_synchronize(hrt_context* ctx);
hrt_status hrt_get_stats(hrt_context* ctx, hrt_stats* out); /* synchronizes */
hrt_status hrt_reset_stats(hrt_context* ctx);
hrt_status hrt_get_diagnostics(hrt_context* ctx, uint64_t* out, uint32_t count); /* synchronizes */
/* Diagnostics (HRT_OPT_COUNTERS = 2): per 8x8 tile of the last trace, row-major over ceil(W/8) x
 * ceil(local_rows/8) tiles, 4 values: shader clocks (slowest work item), bounce iterations, bounce
 * survivor tests, bounce-phase clocks (the frame's critical path is its slowest tile).  count =
 * values (at most 4 x tiles). */
hrt_status hrt_get_tile_profile(hrt_context* ctx, uint64_t* out, uint32_t count);
/* Extension (no reference counterpart): out[i] = hrt_scene_info i for i < count, from the last
 * hrt_set_scene. */
hrt_status hrt_get_scene_info(hrt_context* ctx, uint32_t* out, uint32_t count);

/* On-device ray centres: fills the context's ray buffer with exactly the records
 * hrt_host_create_rays would produce (create_ray_subbuffer, src/raytrace_pipeline.rs:289-338) for
 * the context's width x height, without the host array or its upload.  A later hrt_set_scene may then
 * pass rays == NULL, n_rays == 0 to keep them.  default_jitter (may be NULL) receives :337's value. */
hrt_status hrt_generate_rays(hrt_context* ctx, float camera_focal_length, float viewport_height, const float up[3],
                             float* default_jitter);
/* Copies n (<= width*height) ray records of the context to host memory (verification). */
hrt_status hrt_read_rays(hrt_context* ctx, hrt_ray* out, uint32_t n);

/* Present interop (replaces the reference's image -> texture hand-off,
 * src/raytracing_app.rs:196-227): import memory the presenting API exported as an opaque POSIX fd
 * (Vulkan: VK_KHR_external_memory_fd, vkGetMemoryFdKHR on the staging buffer's memory, size = its
 * allocation size) and map [offset, offset + bytes) into *dev_ptr.  On success the fd belongs to
 * the import.  hrt_read_image(ctx, HRT_IMG_ACCUM, fmt, *dev_ptr, bytes) then writes each frame
 * there device to device.  Imports are released by hrt_release_external_memory or hrt_destroy. */
hrt_status hrt_import_external_memory(hrt_context* ctx, int fd, uint64_t size, uint64_t offset, uint64_t bytes,
                                      void** dev_ptr);
hrt_status hrt_release_external_memory(hrt_context* ctx, void* dev_ptr);

/* ---- the present pass (RenderPassOverFrame::render, src/texture_draw_pipeline.rs:96-157) -------------
 * Writes image info->image_id of the context (Ws x Hs) into the caller's target (info->width x
 * info->height pixels, rows info->pitch bytes apart) as the reference's full-target quad does: nearest
 * filter, flipped vertically (its NDC (-1,-1), the target's top-left, maps to tex (0,1); :28-50), not
 * horizontally.  Target pixel (x, y) takes source texel
 *     sx = ((2x+1) Ws) div (2 Wt),   sy = Hs - 1 - ((2y+1) Hs) div (2 Ht)        (64-bit intermediates)
 * which is dst(x, y) = src(x, Hs-1-y) at equal sizes (DESIGN.md §2 pins the rule, texel edges included).
 * HRT_PRESENT_B8G8R8A8 swaps bytes 0 and 2 of each RGBA8 pixel, HRT_PRESENT_R8G8B8A8 copies it; an
 * HRT_MODE_RGBA32F image is converted channel by channel as hrt_read_image(HRT_FMT_RGBA8) converts it.
 * Bytes of a target row beyond width*4 (pitch padding) are not written.
 *
 * Non-blocking: the pass is enqueued on the context's stream after the work issued so far (deferred
 * combines are folded first; HRT_IMG_TRACE joins and releases the current trace lane like hrt_read_image)
 * and the call returns.  Work issued afterwards is ordered after it, so the target holds the image as
 * of the call whatever is queued behind.  *ticket receives the pass's completion ticket: tickets count
 * up from 1 per context, each a HIP event recorded after the pass.  At most 8 are in flight: a call
 * that finds all 8 unfinished first waits for the oldest.  hrt_synchronize completes every ticket.
 *
 * dst must be memory a kernel may write: inside an import of this context
 * (hrt_import_external_memory), or device, managed or registered (pinned) host memory as
 * hipPointerGetAttributes reports it; dst 4-byte aligned; dst_bytes >= (height-1)*pitch + width*4.
 * Anything else -- pageable host memory included -- is HRT_ERR_INVALID_ARGUMENT, decided on the host
 * before anything is enqueued.
 *
 * The gathered present.  On member 0 (the root, part 0) of an intact hrt_comm_init_all group -- either
 * transport, any world >= 1 -- the source is the group's full width x height image: global row y lives
 * in part (y / row_tile) % parts at local row (y / row_tile / parts) * row_tile + y % row_tile, and the
 * rule above runs with Ws = width and Hs = height (the full height, not local_rows; the parts' padded
 * local rows are never sampled).  The target holds, byte for byte, what hrt_present writes on an
 * unpartitioned context holding the same frame.  The call still only enqueues: every member's block is
 * gathered to the root behind the work issued so far on that member (deferred combines folded first on
 * every member; HRT_IMG_TRACE joins and then releases each member's current trace lane), one kernel on
 * the root's stream reads the gathered blocks and writes the target, and work issued afterwards on any
 * member is ordered after the part of the pass that reads that member's image -- all by streams and
 * events on the device, with no host wait.  Tickets come from the root's sequence; hrt_present_done,
 * hrt_present_wait and hrt_synchronize on the root behave as above, and dst is checked against the
 * root's device and imports.
 * Rejected with HRT_ERR_INVALID_ARGUMENT before anything is enqueued on any member (the message names
 * the reason): a member other than the root, a group with a destroyed member, a context joined with
 * hrt_comm_init (one process per GPU: a present there would be a collective), and a context of a
 * row-tile partition (part_count > 1) with no communicator. */
hrt_status hrt_present(hrt_context* ctx, const hrt_present_info* info, void* dst, uint64_t dst_bytes,
                       uint64_t* ticket);
/* hrt_accumulate(ctx, frame) followed by hrt_present(ctx, info, ...) with info->image_id ==
 * HRT_IMG_ACCUM (any other id is rejected), byte for byte; hrt_stats.accumulates counts it once.  When
 * the target has the image's size and HRT_OPT_DEFER_COMBINE is off, both run as one kernel that folds
 * the pixel, writes the accumulator and writes the target; otherwise as the two passes.
 * On the root of an hrt_comm_init_all group: hrt_accumulate(member, frame) on every member in part order,
 * each on its own stream (every member's hrt_stats.accumulates counts once), then the gathered present of
 * HRT_IMG_ACCUM -- the fold runs on each member's device, the present on the root's. */
hrt_status hrt_accumulate_present(hrt_context* ctx, uint32_t frame, const hrt_present_info* info, void* dst,
                                  uint64_t dst_bytes, uint64_t* ticket);
/* *done = 1 when the pass of `ticket` has finished, else 0 (a poll).  Ticket 0 or one never issued:
 * HRT_ERR_INVALID_ARGUMENT.  A ticket more than 8 behind the newest is done. */
hrt_status hrt_present_done(hrt_context* ctx, uint64_t ticket, uint32_t* done);
/* Blocks until the pass of `ticket` has finished. */
hrt_status hrt_present_wait(hrt_context* ctx, uint64_t ticket);
/* ---- the denoise pass (DESIGN.md §2 S14 pins the arithmetic, §27 the kernels) ----------------------------
 * An edge-avoiding a-trous filter between an image of the context and its consumer: info->iterations passes
 * of a 5 x 5 B3-spline window with taps 1, 2, 4, 8, 16 pixels apart, each tap weighted by its colour
 * distance (sigma_colour) and, with a guide, by the angle between the normals (sigma_normal) and the depth
 * difference relative to the centre's depth (sigma_depth); taps on another surface than the centre's are
 * skipped.  Every byte of the result is defined by S14: the three methods, both libraries and the numpy
 * restatement in tests/denoise_ref.py agree bit for bit.  The data stays float between the passes in either
 * context mode; the source image is never written.
 *
 * guide: NULL (the colour-only filter), or width x height hrt_hit records in memory of the context's device,
 * 16-byte aligned, row-major in trace-image row order -- what hrt_intersect_primary writes for the whole
 * image (x0 = y0 = 0, w = width, h = height) into device memory.
 *
 * Both calls are ordered on the context's stream after the work issued so far (deferred combines are folded
 * first; HRT_IMG_TRACE joins and releases the current trace lane like hrt_read_image) and touch no trace
 * lane's image, hrt_stats, counter or fold record.  Their scratch images (two float4 images and the compact
 * guide, 52 bytes per pixel in all) are allocated by the first call and freed by hrt_destroy.
 *
 * Rejected with HRT_ERR_INVALID_ARGUMENT before anything is enqueued (the message names the reason): a NULL
 * info; iterations 0 or above 5; a sigma that is not finite or not > 0; flags != 0; an unknown method, image
 * id or fmt; a guide that is not memory of the context's device or not 16-byte aligned; a NULL or too small
 * dst; and a context of a row-tile partition (part_count > 1) or one joined to any communicator: a tap's
 * neighbour rows live on another part, and the gathered form of the filter is deliberately out of scope. */

/* ACCUM, 5 iterations, AUTO and the default sigmas (DESIGN.md §27 has the grid they were chosen from). */
void hrt_denoise_defaults(hrt_denoise_info* info);
/* BLOCKING, like hrt_read_image: height x width texels of the filtered image in fmt (hrt_format; RGBA8 is S7's
 * store of each channel with alpha 255, RGBA32F has alpha 1.0f) to host or device memory at dst
 * (bytes >= height * width * 4 or 16). */
hrt_status hrt_denoise(hrt_context* ctx, const hrt_denoise_info* info, const hrt_hit* guide, uint32_t fmt, void* dst,
                       size_t bytes);
/* NON-blocking: the filter, then hrt_present's pass over the filtered float image -- target, dst, dst_bytes and
 * ticket exactly as hrt_present takes them (flip, nearest sampling, byte order, the writable-memory rule, the
 * ticket sequence and its cap of 8 in flight; hrt_present_done, hrt_present_wait and hrt_synchronize apply).
 * target->image_id must equal info->image_id. */
hrt_status hrt_denoise_present(hrt_context* ctx, const hrt_denoise_info* info, const hrt_hit* guide,
                               const hrt_present_info* target, void* dst, uint64_t dst_bytes, uint64_t* ticket);
/* ---- temporal history (DESIGN.md §2 S15 pins the arithmetic, §28 the kernels) -----------------------------
 * The context owns a count image N: one uint32 per pixel, the number of frames that pixel's accumulator texel
 * holds.  It is allocated and zeroed by the first call of any of the four functions below, freed by
 * hrt_destroy, and neither read nor written by anything else (hrt_accumulate, hrt_compute_n, ... keep their
 * single frame number).  hrt_accumulate_history folds the trace image into the accumulator with the pixel's own
 * count as the combiner's frame number; hrt_reproject carries accumulator and counts from the previous view to
 * the current one through the two views' first hits, rejecting (count 0, texel cleared) every pixel whose
 * surface point the previous view did not hold.  Every byte is defined by S15: both libraries and the numpy
 * restatement in tests/history_ref.py agree bit for bit.
 *
 * hrt_reproject, hrt_accumulate_history and hrt_fill_history are NON-blocking, ordered on the context's stream
 * after the work issued so far (deferred combines are folded first).  hrt_accumulate_history joins and releases
 * the current trace lane exactly as hrt_accumulate does and hrt_stats.accumulates counts it once; it appends no
 * fold record.  Nothing else in hrt_stats, no counter, no ticket and no trace image is touched.
 *
 * prev_hits / cur_hits: width x height hrt_hit records in memory of the context's device, 16-byte aligned,
 * row-major in trace-image row order -- what hrt_intersect_primary writes for the whole image.  They are read
 * by the enqueued pass: keep them unchanged until it has run.
 *
 * Rejected with HRT_ERR_INVALID_ARGUMENT before anything is enqueued (the message names the reason): a NULL
 * argument; an unknown filter; flags != 0; a tolerance that is not finite or negative; a min_normal_dot that is
 * not finite; max_history 0 or above HRT_HISTORY_MAX; hit arrays that are not memory of the context's device or
 * not 16-byte aligned; a too small dst; and a context of a row-tile partition (part_count > 1) or one joined to
 * any communicator: a reprojected pixel's source rows live on another part, and the gathered form is
 * deliberately out of scope. */

/* BILINEAR and the default thresholds (DESIGN.md §28 has the grid they were chosen from). */
void hrt_reproject_defaults(hrt_reproject_info* info);
/* Accumulator and count image of the view `prev` become those of the view `cur` (S15). */
hrt_status hrt_reproject(hrt_context* ctx, const hrt_reproject_info* info, const hrt_view* prev, const hrt_hit* prev_hits,
                         const hrt_view* cur, const hrt_hit* cur_hits);
/* Per pixel with count n: n == 0 copies the trace texel (alpha 255 / 1.0f), else the combiner's fold with
 * frame = n; then the count becomes min(n + 1, max_history) (1 <= max_history <= HRT_HISTORY_MAX). */
hrt_status hrt_accumulate_history(hrt_context* ctx, uint32_t max_history);
/* Every pixel's count = count (0: no history). */
hrt_status hrt_fill_history(hrt_context* ctx, uint32_t count);
/* BLOCKING: the count image, height x width uint32 in trace-image row order, to host or device memory at dst
 * (bytes >= height * width * 4). */
hrt_status hrt_read_history(hrt_context* ctx, uint32_t* dst, size_t bytes);

/* ---- object motion in the temporal history (DESIGN.md §2 S21 pins the arithmetic, §36 the kernels) ---------
 * hrt_reproject and hrt_reproject_moments assume that only the camera moved: the current pixel's surface point is
 * looked up at the same world position in the previous view.  hrt_reproject_motion and
 * hrt_reproject_motion_moments are those two calls with a rigid motion per object: a pixel whose current hit is
 * sphere i (kind 1, hrt_hit.index == i) takes motion->spheres[i], one whose hit is a triangle of mesh m (kind 2,
 * hrt_hit.mesh == m) takes motion->meshes[m]; when that entry has HRT_MOTION_MOVING the surface point goes through
 * G to where it was in the previous frame before it is looked up there, and the current normal goes through G's
 * linear part before the normal test.  An index at or past its table's count, an entry with flags == 0 and a
 * miss are static: they take S15's statements, not a multiplication by an identity, so a call whose tables are
 * empty or all static writes hrt_reproject[_moments]' bytes.  Every byte is defined by S21: both libraries and the
 * numpy restatement in tests/motion_ref.py agree bit for bit.
 *
 * The tables are HOST arrays.  They are copied before the call returns: the caller may overwrite or free them at
 * once.  The calls do not wait for the device: the copy goes through a ring of HRT_MOTION_RING pinned staging
 * slots of the context's own (each with its device copy, written by a stream-ordered copy), and a call blocks
 * only when all of them belong to passes that have not run yet -- then for the oldest one (and once more when a
 * slot has to grow for a larger table).  A NULL table with count 0 is allowed.
 *
 * Everything else is hrt_reproject[_moments]': the ordering on the context's stream, the swap of the accumulator,
 * N and M, the statistics, counters, tickets, fold records and trace images that stay untouched, and every
 * rejection (row-tile partitions and communicator-joined contexts included).  Rejected besides, with
 * HRT_ERR_INVALID_ARGUMENT before anything is enqueued (the message names the reason): motion NULL; a count above
 * HRT_MOTION_MAX_OBJECTS; a count that is not 0 with a NULL pointer; an entry with a flag bit other than
 * HRT_MOTION_MOVING; a moving entry with a component of m that is not finite. */
hrt_status hrt_reproject_motion(hrt_context* ctx, const hrt_reproject_info* info, const hrt_motion_tables* motion,
                                const hrt_view* prev, const hrt_hit* prev_hits, const hrt_view* cur,
                                const hrt_hit* cur_hits);
hrt_status hrt_reproject_motion_moments(hrt_context* ctx, const hrt_reproject_info* info,
                                        const hrt_motion_tables* motion, const hrt_view* prev, const hrt_hit* prev_hits,
                                        const hrt_view* cur, const hrt_hit* cur_hits);

/* ---- the variance-guided denoise (DESIGN.md §2 S16 pins the arithmetic, §31 the kernels) ------------------
 * Beside the accumulator and the count image N the context owns a moments image M: two floats per pixel, the
 * running first and second moment (m1, m2) of the luminance of the frames that pixel's accumulator texel
 * holds, float in either context mode.  It is allocated and zeroed by the first call of any function below and
 * freed by hrt_destroy.  hrt_accumulate_history_moments and hrt_reproject_moments are hrt_accumulate_history
 * and hrt_reproject -- the same bytes in the accumulator and in N, the same ordering, lanes and the one count in
 * hrt_stats.accumulates -- and carry M with them: the fold adds the sample (l, l * l) of the trace texel with the
 * pixel's own count, the reprojection carries M through the accepted taps with their weights and clears it
 * where it rejects.  hrt_accumulate_history, hrt_reproject and hrt_fill_history neither read nor write M: a
 * caller who mixes the plain and the moments calls gets moments that describe another accumulator (stale, never
 * out of bounds); nothing polices it.
 *
 * hrt_denoise_variance is hrt_denoise's a-trous filter over HRT_IMG_ACCUM with a per-pixel colour constant: the
 * variance of the accumulated luminance is estimated per pixel -- from M and N where N >= min_history, else from
 * the 7 x 7 neighbourhood of the same surface -- filtered along with the colour, and each pass weighs a tap's
 * colour distance by 1 / (sigma_variance^2 * variance + variance_floor), the variance smoothed over 3 x 3
 * pixels: a settled pixel is left nearly alone, a pixel a move has just uncovered is filtered widely.  Every
 * byte of every result is defined by S16: the three methods, both libraries and the numpy restatement in
 * tests/variance_ref.py agree bit for bit.  guide: as hrt_denoise takes it.  The filter shares hrt_denoise's
 * scratch images; M, the image hrt_reproject_moments writes M' into (swapped with M after the pass, like the
 * accumulator's) and a staging image for a variance_dst in host memory are the context's own.
 *
 * hrt_accumulate_history_moments, hrt_reproject_moments, hrt_fill_moments and hrt_denoise_variance_present are
 * NON-blocking, ordered on the context's stream after the work issued so far (deferred combines are folded
 * first).  No fold record, ticket (but hrt_denoise_variance_present's own), counter, trace image or other field
 * of hrt_stats is touched.
 *
 * Rejected with HRT_ERR_INVALID_ARGUMENT before anything is enqueued (the message names the reason): everything
 * hrt_accumulate_history, hrt_reproject, hrt_denoise and hrt_denoise_present reject; iterations above 5;
 * min_history 0; a sigma or floor that is not finite or not > 0; an unknown method; flags != 0; a too small
 * variance_bytes or moments destination; a target whose image_id is not HRT_IMG_ACCUM; and a context of a
 * row-tile partition or one joined to any communicator. */

/* 5 iterations, AUTO, min_history 4 and the default sigmas (DESIGN.md §31 has the grid they were chosen from). */
void hrt_variance_defaults(hrt_variance_info* info);
/* hrt_accumulate_history, and M <- the fold of the trace texel's (l, l * l) with the pixel's count. */
hrt_status hrt_accumulate_history_moments(hrt_context* ctx, uint32_t max_history);
/* hrt_reproject, and M <- M carried through the same taps; (0, 0) where the pixel is rejected. */
hrt_status hrt_reproject_moments(hrt_context* ctx, const hrt_reproject_info* info, const hrt_view* prev,
                                 const hrt_hit* prev_hits, const hrt_view* cur, const hrt_hit* cur_hits);
/* Every pixel's moments = (m1, m2). */
hrt_status hrt_fill_moments(hrt_context* ctx, float m1, float m2);
/* BLOCKING: the moments image, height x width x 2 floats in trace-image row order, to host or device memory at
 * dst (bytes >= height * width * 8). */
hrt_status hrt_read_moments(hrt_context* ctx, float* dst, size_t bytes);
/* BLOCKING, like hrt_denoise: the filtered accumulator in fmt to host or device memory at dst, and, when
 * variance_dst is not NULL, the filtered variance, height x width floats, to host or device memory there
 * (variance_bytes >= height * width * 4). */
hrt_status hrt_denoise_variance(hrt_context* ctx, const hrt_variance_info* info, const hrt_hit* guide, uint32_t fmt,
                                void* dst, size_t bytes, float* variance_dst, size_t variance_bytes);
/* NON-blocking: the filter, then hrt_present's pass over the filtered float image, with hrt_denoise_present's
 * ticket rules.  target->image_id must be HRT_IMG_ACCUM. */
hrt_status hrt_denoise_variance_present(hrt_context* ctx, const hrt_variance_info* info, const hrt_hit* guide,
                                        const hrt_present_info* target, void* dst, uint64_t dst_bytes, uint64_t* ticket);

/* ---- the first-hit pass ----
 * The whole image's first hits, NON-blocking: enqueued on the context's stream after the work issued so far, so
 * hrt_reproject / hrt_denoise* calls that follow read its result with nothing more to do.  hits: width x height
 * records in memory of the context's device, 16-byte aligned, row-major in trace-image row order; keep the
 * buffer until the pass has run.  The bytes are those hrt_intersect_primary(ctx, pc, 0, 0, width, height, any
 * method, hits, ...) writes (S11: the un-jittered direction, pc's counts, the literal scan for irregular rays),
 * whatever the method here.  The pass touches no trace lane, image, hrt_stats, counter, fold record or ticket; its
 * camera lists are a set of its own (allocated by the first TILES call, dropped by hrt_set_scene), keyed so that a
 * second call from the same camera and counts rebuilds nothing.
 *
 * flags: HRT_FIRST_HITS_COUNT zeroes a context-owned record on the stream and has the kernel add to it; without
 * it no counting code runs.  hrt_get_first_hits_stats (BLOCKING: it synchronizes the stream) returns the last
 * counted call's record, zeros when there was none.
 *
 * HRT_ERR_NO_SCENE without a scene.  Rejected with HRT_ERR_INVALID_ARGUMENT before anything is enqueued: a NULL
 * argument; an unknown method; flag bits other than bit 0; hits that is not memory of the context's device or
 * not 16-byte aligned; a push block whose size or counts the context does not hold; and a context of a row-tile
 * partition or one joined to any communicator (the rule of the pass's consumers). */
hrt_status hrt_first_hits(hrt_context* ctx, const hrt_push_constants* pc, uint32_t method, uint32_t flags, hrt_hit* hits);
hrt_status hrt_get_first_hits_stats(hrt_context* ctx, hrt_first_hits_stats* out);

/* ---- adaptive refinement (DESIGN.md §2 S17 pins the arithmetic, §32 the kernels) ----------------------------
 * New frames only for the pixels whose estimate is still noisy.  hrt_refine_select reads the count image N, the
 * moments image M (both allocated and zeroed by the first call that needs them, as the history calls do) and an
 * optional guide, and marks pixel p with n = N(p):
 *     n >= max_count                  -> not selected (the pixel's budget);
 *     else n < min_history            -> selected (no usable estimate yet);
 *     else                               selected iff  a > tolerance^2 * max(b, luminance_floor)^2,
 * where a is the mean over the window's kept taps q of max(m2(q) - m1(q)^2, 0) / N(q) -- the squared standard
 * error of q's mean luminance -- and b the mean of their m1(q); a tap is kept when it lies inside the image, on
 * p's surface (S14's key of the guide's records; without a guide every key is 0) and has N(q) >= min_history.
 * Pooling keeps a pixel whose own first samples happened to agree (variance 0) in the selection while its
 * neighbours on the surface are noisy.  The mask has hrt_occluded's layout over i = x + y * width: pixel i is bit
 * i & 31 of word i >> 5, ceil(width * height / 32) words, each written in full, the unused bits of the last 0.
 *
 * hrt_refine runs one pass over a mask: for every selected pixel p, with t(p) the texel hrt_trace(ctx, pc) stores
 * at p (the radiance query (pc->cam_pos, pc->rng_offset * 719393 + i, ray centre i) of hrt_radiance, in RGBA8
 * mode through the UNORM8 store), the accumulator, N and -- with HRT_REFINE_MOMENTS -- M at p become exactly
 * what hrt_accumulate_history[_moments](max_history) makes of them from t(p); every other pixel keeps its bytes.
 * Bits of the last word beyond the image are ignored.  HRT_REFINE_QUERIES traces the selected pixels alone, as a
 * compact list through hrt_radiance's kernels (query_method: hrt_query_method, AUTO as hrt_radiance resolves it),
 * and touches no trace lane, trace image, hrt_stats, counter, fold record or ticket.  HRT_REFINE_FRAME is
 * hrt_trace(ctx, pc) -- the frame is left in the trace image and counts in hrt_stats as hrt_trace's -- followed
 * by the masked fold (hrt_stats.accumulates does not count it).  Both give the same accumulator, N and M.
 * BLOCKING: the number of selected pixels comes back to the host to size the launches.  Ordered on the context's
 * stream after the work issued so far (deferred combines are folded first).  With nothing selected nothing is
 * traced and nothing changes (stats: selected 0, method_ran 0).
 *
 * hrt_refine_until: pass k = 0, 1, ... < max_passes selects with the rule; when nothing is selected it stops with
 * *settled = 1; else it refines with pc's rng_offset + k and HRT_REFINE_MOMENTS forced on (the rule reads M).
 * *passes_done = the refinement passes run, *pixel_frames = the sum of their selected counts; settled may be
 * NULL.  The caller chooses pc->rng_offset beyond the frames the history already holds (not policed: a repeated
 * offset folds a sample twice).  BLOCKING.  With HRT_REFINE_AUTO or HRT_REFINE_FRAME the passes' frames go through the
 * trace image and hrt_stats as hrt_trace's do; HRT_REFINE_QUERIES leaves both alone.
 *
 * mask: host memory, or memory of the context's device (then 4-byte aligned).  guide: NULL, or width x height
 * hrt_hit records in memory of the context's device, 16-byte aligned (what hrt_first_hits writes).
 * hrt_refine_select with selected == NULL and a device mask is NON-blocking (stream-ordered); otherwise BLOCKING.
 * The calls' buffers (mask staging, the query, index and result lists: 52 bytes per pixel) belong to the context,
 * are allocated by the first call that needs them and freed by hrt_destroy.
 *
 * HRT_ERR_NO_SCENE without a scene (hrt_refine, hrt_refine_until).  Rejected with HRT_ERR_INVALID_ARGUMENT before
 * anything is enqueued (the message names the reason): a NULL argument (but the optional ones); an unknown
 * method or query method; flag bits beyond HRT_REFINE_MOMENTS; rule->flags != 0; min_history 0; max_count below
 * min_history; radius above 3; a tolerance or floor that is not finite or not > 0; max_history 0 or above
 * HRT_HISTORY_MAX; pc->init; a push block whose size or counts the context does not hold; a misaligned device
 * pointer; a guide that is not memory of the context's device; and a context of a row-tile partition or one
 * joined to any communicator, as the history calls reject them. */

/* min_history 4, max_count 2^24, radius 1, tolerance 0.05, luminance_floor 0.01 (DESIGN.md §32 has the grid). */
void hrt_refine_defaults(hrt_refine_rule* rule);
hrt_status hrt_refine_select(hrt_context* ctx, const hrt_refine_rule* rule, const hrt_hit* guide, uint32_t* mask,
                             uint64_t* selected);
hrt_status hrt_refine(hrt_context* ctx, const hrt_push_constants* pc, const uint32_t* mask, uint32_t max_history,
                      uint32_t method, uint32_t query_method, uint32_t flags, hrt_refine_stats* stats);
hrt_status hrt_refine_until(hrt_context* ctx, const hrt_push_constants* pc, const hrt_refine_rule* rule,
                            const hrt_hit* guide, uint32_t max_history, uint32_t max_passes, uint32_t method,
                            uint32_t flags, uint32_t* passes_done, uint64_t* pixel_frames, uint32_t* settled);

/* ---- tile-masked refinement -----------------------------------------------------------
 * hrt_refine_tiles(mask, frames = F) leaves the accumulator, N and -- with HRT_REFINE_MOMENTS -- M byte for byte
 * as F successive hrt_refine(ctx, pc_f, mask, max_history, HRT_REFINE_FRAME, 0, flags, NULL) calls do, pc_f being
 * pc with rng_offset + f, f = 0 .. F - 1 in order -- but its trace launches run only the 8x8 tiles that hold a
 * selected real pixel (x < width, y < local rows), several frames per launch.  The mask is hrt_refine's in every
 * respect.  The pass runs as hrt_compute_n's launches do: on lane 0's buffers and the context's stream, after the
 * deferred combines and every lane's last trace, at most HRT_OPT_FRAMES_PER_LAUNCH frames per launch through the
 * frame stack.  Every real pixel of a selected tile is traced (the fold stays per pixel under the mask); no pixel
 * of any other tile is.  hrt_stats: traces grows by F, accumulates is unchanged, segments and tri_tests grow by
 * the traced pixels' sums, last_kernel / last_block / last_frames are the last launch's.  No fold record is
 * appended and no ticket is taken.  Afterwards HRT_IMG_TRACE is lane 0's image: the real pixels of the selected
 * tiles hold frame rng_offset + F - 1's texels (exactly hrt_trace's), every other byte of it keeps what it held.
 * Lane 0's tile costs and plan are read, never written: the masked launches plan in buffers of the context's own
 * (allocated by the first call, freed by hrt_destroy), from lane 0's costs where it has them, else from a cost
 * of 1 per tile; a later hrt_trace or hrt_compute_n plans as if the pass had not happened.
 * stats->whole_frame = 1: the launches ran every tile (the same accumulator, N and M; the trace image is then
 * frame rng_offset + F - 1 whole, and a persistent kernel's launches record lane 0's costs as hrt_compute_n's
 * do) -- when the kernel the request resolves to is not persistent, the image has more than 2^22 - 1 tiles, or
 * HRT_OPT_COUNTERS = 2 diagnostics are on.  With nothing selected nothing is enqueued beyond the count, the
 * stats are zero and hrt_stats is untouched.  BLOCKING, as hrt_refine.  Rejected as hrt_refine rejects, before
 * anything is enqueued; also frames 0 or above HRT_REFINE_TILES_MAX_FRAMES.
 *
 * hrt_refine_tiles_until is hrt_refine_until's loop with one hrt_refine_tiles pass of frames_per_pass frames
 * (HRT_REFINE_MOMENTS forced) per selection: pass k starts at rng_offset + k * frames_per_pass, *pixel_frames
 * grows by the selected count x frames_per_pass per pass.  With frames_per_pass = 1 every output and every byte
 * of state is hrt_refine_until(..., HRT_REFINE_FRAME, ...)'s.  The selection is made once per pass, so a pixel
 * can pass rule->max_count by up to frames_per_pass - 1 frames. */
#define HRT_REFINE_TILES_MAX_FRAMES 4096u
hrt_status hrt_refine_tiles(hrt_context* ctx, const hrt_push_constants* pc, const uint32_t* mask, uint32_t max_history,
                            uint32_t frames, uint32_t flags, hrt_refine_tiles_stats* stats);
hrt_status hrt_refine_tiles_until(hrt_context* ctx, const hrt_push_constants* pc, const hrt_refine_rule* rule,
                                  const hrt_hit* guide, uint32_t max_history, uint32_t max_passes,
                                  uint32_t frames_per_pass, uint32_t flags, uint32_t* passes_done,
                                  uint64_t* pixel_frames, uint32_t* settled);
/* ---- guided upsampling ----
 * hrt_upsample shows the context's width x height image at info->width x info->height: a joint-bilateral
 * reconstruction guided by the first hits of both resolutions.  low_hits are the context's own width x height
 * records, high_hits info->width x info->height records in trace-image row order, both in memory of the context's
 * device, 16-byte aligned -- typically hrt_first_hits of this context and of a second context of the target's size.
 * The mapping assumes that both grids come from the same viewport (hrt_host_ray_grid puts pixel centres at
 * (i + 0.5) / W): the caller must give both contexts the same camera, focal length and viewport height.  Nothing
 * polices it.  A target pixel takes the footprint x footprint low texels around its centre, each weighted by a tent
 * and S14's normal and depth weights against the pixel's own high record, taps of another surface key skipped; a
 * pixel that keeps no weight takes hrt_present's nearest texel.  Sizes larger, equal and smaller than the source are
 * all defined.
 *
 * denoise and variance are optional and at most one may be given: that filter runs first over the low image with
 * low_hits as its guide, exactly as hrt_denoise / hrt_denoise_variance run it, and the upsample reads its float
 * result; its image (denoise->image_id; the accumulator for variance) must be info->image_id and all of its own
 * rejections apply.  With neither, the low image is info->image_id's texels as float (S14's C0).
 *
 * hrt_upsample is BLOCKING, like hrt_denoise: it writes height x width texels in fmt (HRT_FMT_RGBA8 by S7's store
 * with alpha 255, HRT_FMT_RGBA32F with alpha 1.0f) to host or device memory -- directly when dst is addressable
 * device memory, else through a context-owned staging image.  hrt_upsample_present is NON-blocking; tickets and
 * the writable-memory rule are hrt_present's; target->width / height must equal info->width / height and
 * target->image_id info->image_id; the target holds what hrt_present's equal-size rule makes of the result,
 * dst(x, y) = U(x, height - 1 - y) in target->format's byte order.  The kernel writes the target directly.
 * Neither changes an image, hrt_stats, a counter, a fold record, N or M; the scratch is the denoise pass's.
 * Rejected with HRT_ERR_INVALID_ARGUMENT before anything is enqueued: a NULL info, low_hits, high_hits or
 * destination; both filters; a footprint other than 2 or 4; flags != 0; a sigma that is not finite or not > 0; a
 * size of 0 or above 16384; an unknown fmt or image id; hit arrays that are not memory of the context's device or
 * not 16-byte aligned; a destination that is too small; a target whose size or image_id disagrees; a context of a
 * row-tile partition or joined to a communicator. */
void hrt_upsample_defaults(hrt_upsample_info* info, uint32_t width, uint32_t height);
hrt_status hrt_upsample(hrt_context* ctx, const hrt_upsample_info* info, const hrt_denoise_info* denoise,
                        const hrt_variance_info* variance, const hrt_hit* low_hits, const hrt_hit* high_hits,
                        uint32_t fmt, void* dst, size_t bytes);
hrt_status hrt_upsample_present(hrt_context* ctx, const hrt_upsample_info* info, const hrt_denoise_info* denoise,
                                const hrt_variance_info* variance, const hrt_hit* low_hits, const hrt_hit* high_hits,
                                const hrt_present_info* target, void* dst, uint64_t dst_bytes, uint64_t* ticket);
/* Work issued on ctx after the call is ordered after everything issued so far on producer's context stream: one
 * event that producer owns, recorded on its stream, and a stream wait on ctx's.  No host wait.  A no-op when the
 * two are the same context; two contexts on different devices are rejected.  (A context that upsamples takes its
 * high-resolution first hits from a second context: this orders the two without hrt_synchronize.) */
hrt_status hrt_order_after(hrt_context* ctx, hrt_context* producer);
/* ---- temporal upsampling ----
 * A context that traces below display size samples a new sub-pixel position of the display grid each frame
 * (hrt_set_ray_grid with hrt_history_phase's offset), and hrt_accumulate_history_from folds each of its trace texels
 * into the display-size history pixel the sample landed in: after nx * ny frames every display pixel has had a
 * sample of its own, and the history converges to what a display-size trace would have produced.
 *
 * hrt_set_ray_grid makes the context's ray centres (first + dx * x) + dy * y, as hrt_host_ray_grid and
 * hrt_generate_rays define them, each operation rounded as written.  NON-blocking, and unlike hrt_generate_rays it
 * never waits on the host: the write runs on the context's stream after every trace in flight on any trace lane and
 * before every trace, first-hit pass, refinement or query issued afterwards (events and stream waits only).  The ray
 * buffer is allocated when the context has none (that one call may synchronise the device); every lane's tile lists
 * are marked stale.  A later hrt_set_scene with rays = NULL keeps the rays.  A grid shifted by (ox, oy) pixels is
 * first' = (first + ox * dx) + oy * dy, computed in float by the caller.  Rejected with HRT_ERR_INVALID_ARGUMENT
 * before anything is enqueued: a NULL argument, a component that is not finite, a context of a row-tile partition or
 * joined to a communicator.
 *
 * hrt_history_phase is host only and pure: the offset of frame k of a ws x hs grid feeding a w x h history.
 * nx = max(1, ceil(w / ws)) in integers, ny likewise from h and hs; a = k mod nx, b = (k div nx) mod ny;
 * *ox = (float(a) + 0.5f) / float(nx) - 0.5f, *oy likewise from b and ny.  Equal sizes and downscaling have one
 * phase, offset 0.  Over any nx * ny consecutive k every target pixel is accepted at least once.  A size of 0
 * counts as one phase; a NULL output is skipped.
 *
 * hrt_accumulate_history_from(ctx, source, info, source_hits, hits): ctx (W x H) owns A, N and M; source (Ws x Hs)
 * owns the most recent trace image T; source == ctx is allowed.  For target pixel p = (x, y), S20:
 *   u = S19's upsample_coord(x, Ws, W) - offset_x, i = floorf(u + 0.5f), dx = fabsf(u - i); v, j, dy likewise;
 *   accepted iff i and j lie inside T (tested in float), dx * float(W) <= 0.5f * float(Ws) and likewise for y (the
 *   source sample lies in p's own pixel) and, with guides, the surface keys of source_hits[j * Ws + i] and
 *   hits[y * W + x] are equal (S14).  Both guides are NULL or both are given.
 *   accepted: exactly one hrt_accumulate_history[_moments] step of p with T(i, j) (M only with HRT_RESOLVE_MOMENTS);
 *   not accepted, HRT_RESOLVE_FILL, N(p) == 0: A(p) = T(ic, jc) with alpha 255 / 1.0f, i and j clamped to the image;
 *   N and M unchanged (a count of 0 still says that A is not history: the next accepted sample overwrites it);
 *   every other pixel keeps A, N and M byte for byte.
 * source == ctx, offsets 0, no guides, flags 0 gives hrt_accumulate_history's bytes; with MOMENTS,
 * hrt_accumulate_history_moments'.
 * NON-blocking.  The kernel runs on ctx's stream, after source's latest trace and its deferred combines and after
 * the work issued so far on ctx; source's next trace into that lane or ring slot waits on the device until the
 * kernel has read T, whatever is called on source in between (an event of the lane's that only this call records).  No host wait.  It changes nothing of source, and of ctx only A, N and, with MOMENTS, M.
 * Rejected with HRT_ERR_INVALID_ARGUMENT before anything is enqueued: a NULL ctx, source or info; contexts on
 * different devices or in different modes; an offset that is not finite or outside [-0.5, 0.5]; max_history outside
 * 1..2^24; unknown flag bits; exactly one guide, or a guide that is not memory of the device or not 16-byte
 * aligned; either context of a row-tile partition or joined to a communicator.  A source other than ctx that has
 * no scene is rejected with HRT_ERR_NO_SCENE (source == ctx is hrt_accumulate_history on that edge too: no such
 * check).  The message of a rejection is ctx's (hrt_last_error). */
void hrt_resolve_defaults(hrt_resolve_info* info); /* offsets 0, max_history 32, HRT_RESOLVE_FILL */
hrt_status hrt_set_ray_grid(hrt_context* ctx, const float first[3], const float dx[3], const float dy[3]);
void hrt_history_phase(uint32_t ws, uint32_t w, uint32_t hs, uint32_t h, uint32_t k, float* ox, float* oy);
hrt_status hrt_accumulate_history_from(hrt_context* ctx, hrt_context* source, const hrt_resolve_info* info,
                                       const hrt_hit* source_hits, const hrt_hit* hits);
/* Test support for the above: device memory exported as an fd (HIP VMM) and the exporter's own
 * mapping of it (*ptr, *size rounded to the allocation granularity); hrt_debug_unmap_memory frees it. */
hrt_status hrt_debug_export_memory(int device, uint64_t bytes, int* fd, void** ptr, uint64_t* size);
hrt_status hrt_debug_unmap_memory(void* ptr, uint64_t size);
/* Test support: the kernels' shared-reciprocal normalize / division and sqrt paths (hrt_math.h) vs
 * the compiler's IEEE sequences, bit for bit, on n hashed inputs of device `device`.
 * out = {normalize mismatches, division mismatches, sqrt mismatches, fast-path cases}. */
hrt_status hrt_debug_math_check(int device, uint32_t n, uint32_t seed, uint64_t out[4]);
/* Test support: the kernels' RNG-domain shortcuts (sqrt of u01 draws and of -2 log(u01), sin/cos of the
 * RNG's angles without the range guard) against the general routines over all 2^32 states.
 * out = {sqrt mismatches, sincos mismatches, Lambertian-shortcut premise or folded-scaling violations
 * (hrt_kernels.hip adjust_dir, hrt_math.h u01_mul), values where the bare hardware square root differs from
 * the correctly rounded one on u01 draws, and on -2 log(u01)}. */
hrt_status hrt_debug_math_check_rng(int device, uint64_t out[5]);
/* Test support: the trace kernel's flattening of a wave's grazing-band lists (64 lanes, lane l's list
 * of n[l] entries starting at entry b0[l]) into 64-slot rounds.  owner_entry[(r * 64 + l) * 2 + {0, 1}] =
 * the owner lane and entry index of slot r * 64 + l (entry 0 past the end), r < rounds <= 4096;
 * *total = the slots in all (the sum of n). */
hrt_status hrt_debug_band_flatten(int device, const uint32_t n[64], const uint32_t b0[64], uint32_t rounds,
                                  uint32_t* owner_entry, uint32_t* total);
/* Test support: the pair traversal's cross-lane LDS handoffs (BUNDLE_WQ's stacks and closest-hit slots) on
 * a scripted run of one wave of 64 lanes over `rounds` <= 1024 rounds.  Slot l starts at seed[l].  Round r:
 * the top min(take[r], depth) stack entries are popped (popped[r * 64 + l] = the entry lane l < take
 * read, else 0xFFFFFFFF; take[r] = nn | tn << 8 pops as a mixed step does: the top nn <= 64 entries go to
 * lanes [0, nn) in stack order, the tn <= 64 - nn entries below them to lanes [nn, nn + tn), each count
 * clamped to what the stack holds); lane l with tgt[r * 64 + l] < 64 reads that slot (seen[r * 64 + l]) and lowers it
 * to val[r * 64 + l] (u64 minimum); then lane l pushes cnt[r * 64 + l] <= 4 entries (r << 16 | l << 8 | k),
 * k-major over the lanes in lane order (while the stack holds at most 8192 - 256).  slots[l] = the final
 * slots, *depth = the final stack depth. */
hrt_status hrt_debug_wq_protocol(int device, uint32_t rounds, const uint32_t* cnt, const uint32_t* take,
                                 const uint32_t* tgt, const uint64_t* val, const uint64_t seed[64], uint32_t* popped,
                                 uint64_t* seen, uint64_t slots[64], uint32_t* depth);
/* Test support, host only: BUNDLE_WQ_L2's LDS plan for an image of n_nodes records with groups of up to
 * `width` and leaves of at most max_leaf triangles, lds_nodes as HRT_OPT_WQ_LDS_NODES and no stack-capacity
 * requests.  out = {L, ncap, tcap, bytes}: the nodes kept in LDS, the per-wave node / triangle pair stack
 * capacities, and the dynamic LDS bytes L x 48 + 16 x (512 + 4 x (ncap + tcap)); all four 0: no fit. */
void hrt_debug_wq_l2_plan(uint32_t n_nodes, uint32_t width, uint32_t max_leaf, int64_t lds_nodes, uint32_t out[4]);
/* Test support: the context's grazing-band structure as the device holds it (hrt_set_scene): the 32 B
 * per-cell records of BUNDLE_WQ (8 words: list start, length, first 12 entries as half-words; rec_words >=
 * 8 x cells), the offsets (off_words >= cells + 1) and the entry words (16-bit entries two to a word unless
 * wide; list_cap >= the words).  A NULL or too small buffer is skipped.  info = {cells, entries, wide,
 * records present}. */
hrt_status hrt_debug_band_records(hrt_context* ctx, uint32_t* rec, uint64_t rec_words, uint32_t* off, uint64_t off_words,
                                  uint32_t* list_words, uint64_t list_cap, uint32_t info[4]);
/* Tuning support: trace lane 0's per-8x8-tile costs as the last persistent launch on it recorded them
 * (shader clocks / 16 summed over the launch's frames; the next launch's plan input), count <= tiles. */
hrt_status hrt_debug_tile_costs(hrt_context* ctx, uint32_t* out, uint32_t count);
/* Test support: the work units (tile x frame) that trace_sky, the sky lane's kernel (HRT_OPT_SKY_LANE), has run on
 * this context since creation or hrt_reset_stats.  Blocking. */
hrt_status hrt_debug_sky_units(hrt_context* ctx, uint64_t* out);
/* Test support: the primary triangle lists of the 8x8 tiles as the tile_lists kernel builds them for a
 * dispatch of pc on this context (camera, ray centres, meshes), into a buffer of its own.  refine = 0: the
 * cap rule alone; refine != 0: the product's lists (the cap rule, then the corner-direction rule per tile
 * and per pixel).  Per tile 66 words: the list length n (<= 64), ok (0: the list overflowed and the
 * kernels cull per iteration; n and the entries are then meaningless), then the n listed triangles in
 * list order as indices into the uploaded triangle buffer (unused words 0xFFFFFFFF).
 * info = {tiles, tiles per row}; a NULL out or words < tiles x 66 fills info only.
 * Blocking; leaves trace lane 0's camera lists rebuilt (the next trace rebuilds its own). */
hrt_status hrt_debug_tile_lists(hrt_context* ctx, const hrt_push_constants* pc, uint32_t refine, uint32_t* out,
                                uint64_t words, uint32_t info[2]);
/* HRT_TIMELINE builds: the last trace launch's item records (4 words each: start, tile list built, end,
 * item | frame << 32 | run << 40 | sky << 47 | wave << 48), at most cap of them copied; *count = the records the launch wrote (<= the
 * HRT_DEBUG_OPT_TIMELINE capacity).  Other builds: HRT_ERR_INVALID_ARGUMENT. */
hrt_status hrt_debug_timeline(hrt_context* ctx, uint64_t* out, uint32_t cap, uint32_t* count);
hrt_status hrt_set_option(hrt_context* ctx, uint32_t key, int64_t value);

/* The context's HIP stream (hipStream_t), for callers that interoperate: work enqueued on it after
 * hrt_accumulate / hrt_compute_n follows them (a trace is joined by the combiner that reads it). */
void* hrt_stream(hrt_context* ctx);

/* Drops the library's process-wide host caches: the grazing-band lists of the last two scenes that
 * hrt_set_scene built (shared by every context of one scene so that a rank group or a test suite builds
 * them once; ~100 MB of host memory each for island, ~130 MB for cave).  Contexts keep working; the next
 * hrt_set_scene of such a scene rebuilds its lists (~0.5 s).  *freed_bytes (may be NULL) receives the
 * bytes released.  Thread-safe. */
hrt_status hrt_release_caches(uint64_t* freed_bytes);

/* Text of the last error on ctx (or of the last hrt_create failure when ctx is NULL). */
const char* hrt_last_error(const hrt_context* ctx);

#ifdef __cplusplus
}
#endif

#endif /* HIP_RAYTRACE_H */
