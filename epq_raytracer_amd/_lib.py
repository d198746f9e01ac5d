"""ctypes binding of libhip_raytrace.so (include/hip_raytrace.h, include/hrt_host.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C epq_raytracer_amd/csrc``.
There is no fallback: if the shared object is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libhip_raytrace.so")
DEBUG_LIB_PATH = os.path.join(_HERE, "lib", "libhip_raytrace_debug.so")  # -DHRT_DEBUG_OPTIONS (tests, tools)

# ---- std430 records (assets/raytracing.glsl:51-153) as numpy dtypes + ctypes structs ----------

MATERIAL_DTYPE = np.dtype([("colour", "<f4", 4), ("emission", "<f4", 4), ("settings", "<f4", 4)])
RAY_DTYPE = np.dtype([("sample_centre", "<f4", 4)])
SPHERE_DTYPE = np.dtype([("centre", "<f4", 3), ("radius", "<f4"), ("material", MATERIAL_DTYPE)])
TRIANGLE_DTYPE = np.dtype([("a", "<f4", 4), ("edge_one", "<f4", 4), ("edge_two", "<f4", 4), ("normal", "<f4", 4)])
MESH_DTYPE = np.dtype([("min_point", "<f4", 3), ("first_index", "<u4"), ("max_point", "<f4", 3), ("len", "<u4"),
                       ("material", MATERIAL_DTYPE)])
assert MATERIAL_DTYPE.itemsize == 48 and RAY_DTYPE.itemsize == 16 and SPHERE_DTYPE.itemsize == 64
assert TRIANGLE_DTYPE.itemsize == 64 and MESH_DTYPE.itemsize == 80


class PushConstants(ctypes.Structure):
    """raytrace_shader::PushConstants (assets/raytracing.glsl:135-153), 124 bytes."""

    _fields_ = [
        ("cam_pos", c_float * 4),
        ("cam_alignment_mat", c_float * 16),
        ("num_rays", c_int32),
        ("num_spheres", c_int32),
        ("num_meshes", c_int32),
        ("num_samples", c_int32),
        ("jitter_size", c_float),
        ("max_bounces", c_int32),
        ("use_environment_light", c_uint32),
        ("rng_offset", c_uint32),
        ("init", c_uint32),
        ("width", c_uint32),
        ("height", c_uint32),
    ]


assert ctypes.sizeof(PushConstants) == 124


class CreateInfo(ctypes.Structure):
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("device", c_int32), ("mode", c_uint32),
                ("row_tile", c_uint32), ("part_index", c_uint32), ("part_count", c_uint32)]


class Layout(ctypes.Structure):
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("local_rows", c_uint32), ("row_tile", c_uint32),
                ("part_index", c_uint32), ("part_count", c_uint32), ("mode", c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [("segments", c_uint64), ("tri_tests", c_uint64), ("traces", c_uint64), ("accumulates", c_uint64),
                ("last_trace_ms", c_float), ("total_trace_ms", c_float), ("wave_steps", c_uint64),
                ("last_kernel", c_uint32), ("last_block", c_uint32), ("last_frames", c_uint32),
                ("reserved", c_uint32)]


class PresentInfo(ctypes.Structure):
    """hrt_present_info: the target of one present pass (24 bytes)."""

    _fields_ = [("image_id", c_uint32), ("format", c_uint32), ("width", c_uint32), ("height", c_uint32),
                ("pitch", c_uint32), ("flags", c_uint32)]


assert ctypes.sizeof(PresentInfo) == 24


class FoldRecord(ctypes.Structure):
    """hrt_fold_record: what one fold did to the displayed image (24 bytes)."""

    _fields_ = [("frame", c_uint32), ("changed_pixels", c_uint32), ("max_delta", c_uint32), ("reserved", c_uint32),
                ("abs_delta_sum", c_uint64)]


class SettleRule(ctypes.Structure):
    """hrt_settle_rule: when hrt_compute_until stops (16 bytes)."""

    _fields_ = [("max_changed_pixels", c_uint32), ("max_delta", c_uint32), ("quiet_frames", c_uint32),
                ("flags", c_uint32)]


assert ctypes.sizeof(FoldRecord) == 24 and ctypes.sizeof(SettleRule) == 16
FOLD_RECORD_DTYPE = np.dtype([("frame", "<u4"), ("changed_pixels", "<u4"), ("max_delta", "<u4"), ("reserved", "<u4"),
                              ("abs_delta_sum", "<u8")])
assert FOLD_RECORD_DTYPE.itemsize == 24
FOLD_RECORD_RING = 1024      # HRT_FOLD_RECORD_RING
RGBA8_FREEZE_FRAME = 510     # HRT_RGBA8_FREEZE_FRAME
RULE_ANY = 0xFFFFFFFF        # a settle-rule bound that is disabled


class RayQuery(ctypes.Structure):
    """hrt_ray_query: one caller ray (32 bytes)."""

    _fields_ = [("origin", c_float * 3), ("t_max", c_float), ("direction", c_float * 3), ("reserved", c_uint32)]


class Hit(ctypes.Structure):
    """hrt_hit: the closest hit of one ray (32 bytes)."""

    _fields_ = [("t", c_float), ("kind", c_uint32), ("index", c_uint32), ("mesh", c_uint32), ("normal", c_float * 3),
                ("reserved", c_uint32)]


class QueryStats(ctypes.Structure):
    """hrt_query_stats: what one hrt_intersect / hrt_intersect_primary call ran (24 bytes)."""

    _fields_ = [("method_ran", c_uint32), ("reserved", c_uint32), ("scan_rays", c_uint64), ("tri_tests", c_uint64)]


class OcclusionStats(ctypes.Structure):
    """hrt_occlusion_stats: what one hrt_occluded call ran (32 bytes)."""

    _fields_ = [("method_ran", c_uint32), ("reserved", c_uint32), ("scan_rays", c_uint64), ("tri_tests", c_uint64),
                ("occluded", c_uint64)]


assert ctypes.sizeof(OcclusionStats) == 32


class RadianceStats(ctypes.Structure):
    """hrt_radiance_stats: what one hrt_radiance call ran (32 bytes)."""

    _fields_ = [("method_ran", c_uint32), ("reserved", c_uint32), ("scan_segments", c_uint64), ("segments", c_uint64),
                ("tri_tests", c_uint64)]


assert ctypes.sizeof(RadianceStats) == 32
RADIANCE_QUERY_DTYPE = np.dtype([("origin", "<f4", 3), ("seed", "<u4"), ("centre", "<f4", 3), ("reserved", "<u4")])
assert RADIANCE_QUERY_DTYPE.itemsize == 32
assert ctypes.sizeof(RayQuery) == 32 and ctypes.sizeof(Hit) == 32 and ctypes.sizeof(QueryStats) == 24
RAY_QUERY_DTYPE = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("kind", "<u4"), ("index", "<u4"), ("mesh", "<u4"), ("normal", "<f4", 3),
                      ("reserved", "<u4")])
assert RAY_QUERY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 32
QUERY_AUTO, QUERY_SCAN, QUERY_BVH, QUERY_PAIRS = 0, 1, 2, 3  # hrt_query_method
QUERY_NAMES = {0: "auto", 1: "scan", 2: "bvh", 3: "pairs"}
HIT_MISS, HIT_SPHERE, HIT_TRIANGLE = 0, 1, 2  # hrt_hit.kind
HIT_NONE = 0xFFFFFFFF  # hrt_hit.index / mesh of a miss


class DenoiseInfo(ctypes.Structure):
    """hrt_denoise_info: one denoise pass (32 bytes)."""

    _fields_ = [("image_id", c_uint32), ("iterations", c_uint32), ("method", c_uint32), ("flags", c_uint32),
                ("sigma_colour", c_float), ("sigma_normal", c_float), ("sigma_depth", c_float), ("reserved", c_uint32)]


assert ctypes.sizeof(DenoiseInfo) == 32
DENOISE_AUTO, DENOISE_DIRECT, DENOISE_TILED = 0, 1, 2  # hrt_denoise_method
DENOISE_NAMES = {0: "auto", 1: "direct", 2: "tiled"}
DEBUG_DENOISE_DENSE, DEBUG_DENOISE_LATTICE = 3, 4  # libhip_raytrace_debug.so only
DENOISE_MAX_ITERATIONS = 5  # steps 1, 2, 4, 8, 16
DENOISE_SIGMAS = (8.0, 0.25, 0.5)  # HRT_DENOISE_SIGMA_COLOUR / _NORMAL / _DEPTH (hrt_denoise_defaults)


class View(ctypes.Structure):
    """hrt_view: a camera and the affine grid of its ray centres (128 bytes)."""

    _fields_ = [("cam_pos", c_float * 4), ("cam_alignment_mat", c_float * 16), ("grid_first", c_float * 4),
                ("grid_dx", c_float * 4), ("grid_dy", c_float * 4)]


class ReprojectInfo(ctypes.Structure):
    """hrt_reproject_info: one reprojection (32 bytes)."""

    _fields_ = [("filter", c_uint32), ("flags", c_uint32), ("depth_tolerance", c_float), ("min_normal_dot", c_float),
                ("reserved", c_uint32 * 4)]


assert ctypes.sizeof(View) == 128 and ctypes.sizeof(ReprojectInfo) == 32
REPROJECT_NEAREST, REPROJECT_BILINEAR = 0, 1  # hrt_reproject_filter
REPROJECT_NAMES = {0: "nearest", 1: "bilinear"}
REPROJECT_DEFAULTS = (0.02, 0.9)  # HRT_REPROJECT_DEPTH_TOLERANCE / _MIN_NORMAL_DOT (hrt_reproject_defaults)
HISTORY_MAX = 1 << 24  # HRT_HISTORY_MAX: the largest max_history of hrt_accumulate_history


class Motion(ctypes.Structure):
    """hrt_motion: one object's rigid motion between two frames (64 bytes) -- m is the column-major 3x4 [L | b] with
    previous world point = L * current world point + b."""

    _fields_ = [("m", c_float * 12), ("flags", c_uint32), ("reserved", c_uint32 * 3)]


class MotionTables(ctypes.Structure):
    """hrt_motion_tables: the host tables of one hrt_reproject_motion call (32 bytes)."""

    _fields_ = [("spheres", ctypes.c_void_p), ("n_spheres", c_uint32), ("meshes", ctypes.c_void_p), ("n_meshes", c_uint32)]


assert ctypes.sizeof(Motion) == 64 and ctypes.sizeof(MotionTables) == 32
MOTION_MOVING = 1  # HRT_MOTION_MOVING
MOTION_MAX_OBJECTS = 65536  # HRT_MOTION_MAX_OBJECTS
MOTION_RING = 4  # HRT_MOTION_RING: calls in flight before hrt_reproject_motion waits for the oldest pass


class VarianceInfo(ctypes.Structure):
    """hrt_variance_info: one variance-guided denoise pass (32 bytes)."""

    _fields_ = [("iterations", c_uint32), ("method", c_uint32), ("flags", c_uint32), ("min_history", c_uint32),
                ("sigma_variance", c_float), ("variance_floor", c_float), ("sigma_normal", c_float),
                ("sigma_depth", c_float)]


assert ctypes.sizeof(VarianceInfo) == 32
VARIANCE_AUTO, VARIANCE_DIRECT, VARIANCE_TILED = 0, 1, 2  # hrt_variance_method
VARIANCE_NAMES = {0: "auto", 1: "direct", 2: "tiled"}
VARIANCE_SIGMA, VARIANCE_FLOOR, VARIANCE_MIN_HISTORY = 4.0, 1e-10, 4  # HRT_VARIANCE_SIGMA / _FLOOR / _MIN_HISTORY
VARIANCE_MAX_ITERATIONS = 5  # steps 1, 2, 4, 8, 16 (0 iterations: the source and the variance estimate)


class UpsampleInfo(ctypes.Structure):
    """hrt_upsample_info: one guided upsample (32 bytes)."""

    _fields_ = [("image_id", c_uint32), ("width", c_uint32), ("height", c_uint32), ("footprint", c_uint32),
                ("flags", c_uint32), ("sigma_normal", c_float), ("sigma_depth", c_float), ("reserved", c_uint32)]


assert ctypes.sizeof(UpsampleInfo) == 32
UPSAMPLE_FOOTPRINT = 2  # HRT_UPSAMPLE_FOOTPRINT (hrt_upsample_defaults)
UPSAMPLE_MAX_DIM = 16384  # the largest width / height of a result


class ResolveInfo(ctypes.Structure):
    """hrt_resolve_info: one fold across resolutions (32 bytes)."""

    _fields_ = [("offset_x", c_float), ("offset_y", c_float), ("max_history", c_uint32), ("flags", c_uint32),
                ("reserved", c_uint32 * 4)]


assert ctypes.sizeof(ResolveInfo) == 32
RESOLVE_FILL, RESOLVE_MOMENTS = 1, 2  # HRT_RESOLVE_* (flags of hrt_resolve_info)
RESOLVE_MAX_HISTORY = 32  # hrt_resolve_defaults' max_history


class FirstHitsStats(ctypes.Structure):
    """hrt_first_hits_stats: what the last counted hrt_first_hits call ran (48 bytes)."""

    _fields_ = [("method_ran", c_uint32), ("reserved", c_uint32), ("tiles", c_uint32), ("tiles_listed", c_uint32),
                ("tiles_empty", c_uint32), ("tiles_fallback", c_uint32), ("scan_rays", c_uint64),
                ("tri_tests", c_uint64), ("entries_tested", c_uint64)]


assert ctypes.sizeof(FirstHitsStats) == 48
FIRST_HITS_AUTO, FIRST_HITS_TILES, FIRST_HITS_QUERY = 0, 1, 2  # hrt_first_hits_method
FIRST_HITS_NAMES = {0: "auto", 1: "tiles", 2: "query"}
FIRST_HITS_COUNT = 1  # HRT_FIRST_HITS_COUNT (flags bit 0)



class RefineRule(ctypes.Structure):
    """hrt_refine_rule: which pixels a refinement pass selects (32 bytes)."""

    _fields_ = [("min_history", c_uint32), ("max_count", c_uint32), ("radius", c_uint32), ("flags", c_uint32),
                ("tolerance", c_float), ("luminance_floor", c_float), ("reserved", c_uint32 * 2)]


class RefineStats(ctypes.Structure):
    """hrt_refine_stats: what one hrt_refine pass ran (48 bytes)."""

    _fields_ = [("method_ran", c_uint32), ("query_method_ran", c_uint32), ("selected", c_uint64),
                ("scan_segments", c_uint64), ("segments", c_uint64), ("tri_tests", c_uint64), ("reserved", c_uint64)]


assert ctypes.sizeof(RefineRule) == 32 and ctypes.sizeof(RefineStats) == 48
REFINE_AUTO, REFINE_QUERIES, REFINE_FRAME = 0, 1, 2  # hrt_refine_method
REFINE_NAMES = {0: "auto", 1: "queries", 2: "frame"}
REFINE_MOMENTS = 1  # HRT_REFINE_MOMENTS (flags bit 0 of hrt_refine / hrt_refine_until)
# HRT_REFINE_MIN_HISTORY / _MAX_COUNT / _RADIUS / _TOLERANCE / _FLOOR (hrt_refine_defaults)
REFINE_MIN_HISTORY, REFINE_MAX_COUNT, REFINE_RADIUS, REFINE_TOLERANCE, REFINE_FLOOR = 4, 1 << 24, 1, 0.05, 0.01
REFINE_MAX_RADIUS = 3


class RefineTilesStats(ctypes.Structure):
    """hrt_refine_tiles_stats: what one hrt_refine_tiles pass ran (40 bytes)."""

    _fields_ = [("kernel_ran", c_uint32), ("whole_frame", c_uint32), ("tiles", c_uint32), ("tiles_selected", c_uint32),
                ("items", c_uint32), ("reserved", c_uint32), ("selected", c_uint64), ("pixels_traced", c_uint64)]


assert ctypes.sizeof(RefineTilesStats) == 40
REFINE_TILES_MAX_FRAMES = 4096  # HRT_REFINE_TILES_MAX_FRAMES

ABI_VERSION = 6  # HRT_ABI_VERSION this binding's signatures describe
TILE_LIST_WORDS = 66  # hrt_debug_tile_lists: n, ok, 64 entries per tile
HRT_OK = 0
STATUS_NAMES = {0: "HRT_OK", 1: "HRT_ERR_INVALID_ARGUMENT", 2: "HRT_ERR_NO_DEVICE", 3: "HRT_ERR_OUT_OF_MEMORY",
                4: "HRT_ERR_NO_SCENE", 5: "HRT_ERR_HIP", 6: "HRT_ERR_IO", 7: "HRT_ERR_COMM"}
ERR_COMM = 7
MODE_RGBA8, MODE_RGBA32F = 0, 1
IMG_TRACE, IMG_ACCUM = 0, 1
IMG_LOCAL = 0x100  # flag: this context's local rows, never the collective gather
FMT_RGBA8, FMT_RGBA32F = 0, 1
PRESENT_B8G8R8A8, PRESENT_R8G8B8A8 = 0, 1  # hrt_present_format
PRESENT_RING = 8  # present tickets in flight per context
OPT_KERNEL_VARIANT, OPT_COUNTERS, OPT_SECONDARY_BATCH, OPT_BVH_LEAF_SIZE = 1, 2, 3, 4
OPT_SPLIT, OPT_SPLIT_FACTOR, OPT_PRIORITY, OPT_GRID_CUS, OPT_COOP, OPT_WQ_NODE_CAP, OPT_PROBE = 5, 6, 7, 8, 9, 10, 11
OPT_FRAMES_PER_LAUNCH, OPT_OVERLAP, OPT_BUSY_SPLIT, OPT_BVH_WIDTH, OPT_WQ_NODE_RADIUS = 12, 13, 14, 15, 16
OPT_COMM_TIMEOUT_MS, OPT_DEFER_COMBINE, OPT_FOLD_RECORDS = 17, 18, 19
OPT_SKY_LANE = 20  # BUNDLE_WQ: sky items on trace_sky beside the main kernel (-1 auto, 0 off, 1 on)
OPT_WQ_LDS_NODES = 21  # BUNDLE_WQ_L2: nodes of the breadth-first image kept in LDS (-1 auto, 0 none, n)
OPT_PRIMARY_BATCH = 22  # fused loop: primary segments join a bounce batch's trip from this many ready lanes (0 auto)
DEBUG_OPT_FAIL_ALLOC = 1001  # libhip_raytrace_debug.so only
DEBUG_OPT_WQ_TRI_CAP = 1002  # libhip_raytrace_debug.so only
DEBUG_OPT_GRAB_RUNS = 1003  # libhip_raytrace_debug.so only
DEBUG_OPT_TIMELINE = 1004  # builds with -DHRT_TIMELINE=1 only (tools/timeline.py)
DEBUG_OPT_STACK_LIMIT = 1005  # libhip_raytrace_debug.so only
COMM_ID_BYTES = 128
COMM_NONE, COMM_RCCL, COMM_RCCL_GROUP, COMM_DEVICE_COPY = 0, 1, 2, 3
# hrt_kernel (include/hip_raytrace.h)
KERNEL_AUTO, KERNEL_LITERAL, KERNEL_BRUTE, KERNEL_BRUTE_LDS, KERNEL_BUNDLE, KERNEL_BUNDLE_CULL = 0, 1, 2, 3, 4, 5
KERNEL_BUNDLE_BVH, KERNEL_BUNDLE_CULL_LDS, KERNEL_BUNDLE_BVH_LDS, KERNEL_BUNDLE_WQ = 6, 7, 8, 9
KERNEL_BUNDLE_WQ_L2 = 10  # BUNDLE_WQ with the node image in global memory / L2 (never picked by AUTO)
# kernel symbol (as rocprofv3 names it) of a resolved hrt_kernel + workgroup size
NODE_RADIUS_MARGIN_MILLI = 100  # auto HRT_OPT_WQ_NODE_RADIUS: per-node R above this bvh_margin_milli (hrt_bvh.h)


def wq_node_radius(scene_info: dict, option: int = 0) -> bool:
    """Whether BUNDLE_WQ runs its per-node-radius kernel (trace_bundle_wq_nr) for this scene."""
    return option == 2 or (option == 0 and scene_info.get("bvh_margin_milli", 0) > NODE_RADIUS_MARGIN_MILLI)


def kernel_symbol(kernel: int, block: int, diag: bool = False, node_r: bool = False) -> str:
    d = "true" if diag else "false"
    if kernel == 9 and node_r:
        return f"void hrt::trace_bundle_wq_nr<{d}>(hrt::TraceParams)"
    if kernel == 10 and node_r:
        return f"void hrt::trace_bundle_wq_l2_nr<{d}>(hrt::TraceParams)"
    if kernel in (1, 2, 3):
        return "hrt::" + {1: "trace_literal", 2: "trace_brute", 3: "trace_brute_lds"}[kernel] + "(hrt::TraceParams)"
    if kernel == 7:
        return f"void hrt::trace_bundle_cull_lds<{block}, {d}>(hrt::TraceParams)"
    name = {4: "trace_bundle", 5: "trace_bundle_cull", 6: "trace_bundle_bvh", 8: "trace_bundle_bvh_lds",
            9: "trace_bundle_wq", 10: "trace_bundle_wq_l2"}.get(kernel, "?")
    return f"void hrt::{name}<{d}>(hrt::TraceParams)"


KERNEL_NAMES = {0: "auto", 1: "literal", 2: "brute", 3: "brute_lds", 4: "bundle", 5: "bundle_cull", 6: "bundle_bvh",
                7: "bundle_cull_lds", 8: "bundle_bvh_lds", 9: "bundle_wq", 10: "bundle_wq_l2"}
DIAG_NAMES = ("primary_iters", "primary_considered", "primary_survivors", "bounce_iters", "bounce_considered",
              "bounce_survivors", "bounce_lanes", "bvh_visits", "bvh_prim_tests", "bvh_band_tests", "primary_cycles", "bounce_cycles",
              "shade_cycles", "bounce_stage2", "bounce_front", "bvh_trips",
              "bvh_leaf_trips", "band_scan_max", "band_scan_len", "sky_items", "sky_cycles",
              "primary_lanes", "loop_iters", "live_lanes", "wq_steps_16", "wq_steps_32", "wq_steps_48",
              "wq_steps_64", "wq_members", "dir_lanes", "primary_deferred", "batch_only_iters")
SCENE_INFO_NAMES = ("bvh_nodes", "bvh_prims", "bvh_irregular", "bvh_never", "bvh_built", "bvh_band_entries",
                    "bvh_sah_milli", "bvh_margin_milli")

# Every symbol include/*.h declares (tests/test_abi.py checks the export table against this).
EXPORTED_SYMBOLS = (
    "hrt_abi_version", "hrt_build_id", "hrt_debug_build", "hrt_debug_check_guards", "hrt_create", "hrt_destroy", "hrt_set_scene", "hrt_trace", "hrt_accumulate", "hrt_compute_n",
    "hrt_compute_until", "hrt_get_fold_records", "hrt_intersect", "hrt_intersect_primary", "hrt_occluded", "hrt_radiance",
    "hrt_first_hits", "hrt_get_first_hits_stats",
    "hrt_read_image", "hrt_load_accumulator", "hrt_get_layout", "hrt_synchronize", "hrt_get_stats", "hrt_reset_stats", "hrt_set_option",
    "hrt_get_diagnostics", "hrt_get_tile_profile", "hrt_get_scene_info", "hrt_generate_rays", "hrt_read_rays",
    "hrt_import_external_memory", "hrt_release_external_memory",
    "hrt_denoise_defaults", "hrt_denoise", "hrt_denoise_present",
    "hrt_reproject_defaults", "hrt_reproject", "hrt_accumulate_history", "hrt_fill_history", "hrt_read_history",
    "hrt_variance_defaults", "hrt_accumulate_history_moments", "hrt_reproject_moments", "hrt_fill_moments",
    "hrt_read_moments", "hrt_denoise_variance", "hrt_denoise_variance_present",
    "hrt_reproject_motion", "hrt_reproject_motion_moments", "hrt_host_motion_between",
    "hrt_refine_defaults", "hrt_refine_select", "hrt_refine", "hrt_refine_until",
    "hrt_refine_tiles", "hrt_refine_tiles_until",
    "hrt_upsample_defaults", "hrt_upsample", "hrt_upsample_present", "hrt_order_after",
    "hrt_resolve_defaults", "hrt_set_ray_grid", "hrt_history_phase", "hrt_accumulate_history_from",
    "hrt_present", "hrt_accumulate_present", "hrt_present_done", "hrt_present_wait", "hrt_debug_export_memory", "hrt_debug_unmap_memory", "hrt_debug_math_check", "hrt_debug_math_check_rng", "hrt_debug_band_flatten", "hrt_debug_wq_protocol",
    "hrt_debug_timeline", "hrt_debug_band_records", "hrt_debug_tile_costs", "hrt_debug_sky_units",
    "hrt_debug_tile_lists",
    "hrt_stream", "hrt_release_caches", "hrt_last_error", "hrt_comm_unique_id", "hrt_comm_init", "hrt_comm_init_all", "hrt_comm_info",
    "hrt_host_create_rays", "hrt_host_ray_grid", "hrt_host_view_matrix", "hrt_host_transform_meshes",
    "hrt_debug_bvh_build", "hrt_debug_bvh_wq_nodes", "hrt_debug_bvh_wq_nodes_bfs", "hrt_debug_wq_l2_plan",
    "hrt_obj_load", "hrt_obj_num_meshes", "hrt_obj_mesh", "hrt_obj_free",
)


class HrtError(RuntimeError):
    """A non-OK hrt_status (the reference would have panicked in .unwrap())."""

    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where} failed: {STATUS_NAMES.get(status, status)}{': ' + detail if detail else ''}")


_libs = {}


def load(debug: bool = False) -> ctypes.CDLL:
    """Load libhip_raytrace.so, or with debug=True libhip_raytrace_debug.so (the same objects with the
    diagnostics-only options compiled in).  Raises if the library has not been built."""
    if debug in _libs:
        return _libs[debug]
    # HRT_LIB: A/B builds of the same ABI (tools/kbench.py experiments)
    path = DEBUG_LIB_PATH if debug else os.environ.get("HRT_LIB", LIB_PATH)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                           " or `make -C epq_raytracer_amd/csrc` (no CPU fallback exists)")
    lib = ctypes.CDLL(path)
    lib.hrt_abi_version.restype = c_uint32
    lib.hrt_abi_version.argtypes = []
    if lib.hrt_abi_version() != ABI_VERSION:  # the signatures below would bind shifted arguments
        raise RuntimeError(f"{path} implements HRT_ABI_VERSION {lib.hrt_abi_version()}, this binding "
                           f"{ABI_VERSION}: rebuild it (make -C epq_raytracer_amd/csrc)")
    P = c_void_p
    sig = {
        "hrt_abi_version": (c_uint32, []),
        "hrt_debug_build": (c_uint32, []),
        "hrt_build_id": (c_char_p, []),
        "hrt_debug_check_guards": (c_int32, [P, POINTER(c_uint32), POINTER(c_uint32)]),
        "hrt_comm_unique_id": (c_int32, [P]),
        "hrt_comm_init": (c_int32, [P, P, c_uint32, c_uint32]),
        "hrt_comm_init_all": (c_int32, [P, c_uint32]),
        "hrt_comm_info": (c_int32, [P, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
        "hrt_create": (c_int32, [POINTER(CreateInfo), POINTER(c_void_p)]),
        "hrt_destroy": (None, [P]),
        "hrt_set_scene": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, P, c_uint32]),
        "hrt_trace": (c_int32, [P, POINTER(PushConstants)]),
        "hrt_accumulate": (c_int32, [P, c_uint32]),
        "hrt_compute_n": (c_int32, [P, POINTER(PushConstants), c_uint32]),
        "hrt_compute_until": (c_int32, [P, POINTER(PushConstants), c_uint32, POINTER(SettleRule), POINTER(c_uint32),
                                        POINTER(c_uint32)]),
        "hrt_get_fold_records": (c_int32, [P, P, c_uint32, POINTER(c_uint32), POINTER(c_uint64)]),
        "hrt_intersect": (c_int32, [P, P, c_uint32, c_uint32, P, POINTER(QueryStats)]),
        "hrt_intersect_primary": (c_int32, [P, POINTER(PushConstants), c_uint32, c_uint32, c_uint32, c_uint32, c_uint32,
                                            P, POINTER(QueryStats)]),
        "hrt_first_hits": (c_int32, [P, POINTER(PushConstants), c_uint32, c_uint32, P]),
        "hrt_get_first_hits_stats": (c_int32, [P, POINTER(FirstHitsStats)]),
        "hrt_occluded": (c_int32, [P, P, c_uint32, c_uint32, P, POINTER(OcclusionStats)]),
        "hrt_radiance": (c_int32, [P, POINTER(PushConstants), P, c_uint32, c_uint32, P, POINTER(RadianceStats)]),
        "hrt_read_image": (c_int32, [P, c_uint32, c_uint32, P, c_size_t]),
        "hrt_load_accumulator": (c_int32, [P, c_uint32, P, c_size_t]),
        "hrt_get_layout": (c_int32, [P, POINTER(Layout)]),
        "hrt_synchronize": (c_int32, [P]),
        "hrt_get_stats": (c_int32, [P, POINTER(Stats)]),
        "hrt_reset_stats": (c_int32, [P]),
        "hrt_get_diagnostics": (c_int32, [P, P, c_uint32]),
        "hrt_get_scene_info": (c_int32, [P, P, c_uint32]),
        "hrt_get_tile_profile": (c_int32, [P, P, c_uint32]),
        "hrt_generate_rays": (c_int32, [P, c_float, c_float, POINTER(c_float), POINTER(c_float)]),
        "hrt_read_rays": (c_int32, [P, P, c_uint32]),
        "hrt_import_external_memory": (c_int32, [P, c_int32, c_uint64, c_uint64, c_uint64, POINTER(c_void_p)]),
        "hrt_release_external_memory": (c_int32, [P, P]),
        "hrt_present": (c_int32, [P, POINTER(PresentInfo), P, c_uint64, POINTER(c_uint64)]),
        "hrt_accumulate_present": (c_int32, [P, c_uint32, POINTER(PresentInfo), P, c_uint64, POINTER(c_uint64)]),
        "hrt_denoise_defaults": (None, [POINTER(DenoiseInfo)]),
        "hrt_denoise": (c_int32, [P, POINTER(DenoiseInfo), P, c_uint32, P, c_size_t]),
        "hrt_denoise_present": (c_int32, [P, POINTER(DenoiseInfo), P, POINTER(PresentInfo), P, c_uint64,
                                          POINTER(c_uint64)]),
        "hrt_reproject_defaults": (None, [POINTER(ReprojectInfo)]),
        "hrt_reproject": (c_int32, [P, POINTER(ReprojectInfo), POINTER(View), P, POINTER(View), P]),
        "hrt_accumulate_history": (c_int32, [P, c_uint32]),
        "hrt_fill_history": (c_int32, [P, c_uint32]),
        "hrt_read_history": (c_int32, [P, P, c_size_t]),
        "hrt_refine_defaults": (None, [POINTER(RefineRule)]),
        "hrt_refine_select": (c_int32, [P, POINTER(RefineRule), P, P, POINTER(c_uint64)]),
        "hrt_refine": (c_int32, [P, POINTER(PushConstants), P, c_uint32, c_uint32, c_uint32, c_uint32, POINTER(RefineStats)]),
        "hrt_refine_until": (c_int32, [P, POINTER(PushConstants), POINTER(RefineRule), P, c_uint32, c_uint32, c_uint32,
                                       c_uint32, POINTER(c_uint32), POINTER(c_uint64), POINTER(c_uint32)]),
        "hrt_refine_tiles": (c_int32, [P, POINTER(PushConstants), P, c_uint32, c_uint32, c_uint32, POINTER(RefineTilesStats)]),
        "hrt_refine_tiles_until": (c_int32, [P, POINTER(PushConstants), POINTER(RefineRule), P, c_uint32, c_uint32, c_uint32,
                                             c_uint32, POINTER(c_uint32), POINTER(c_uint64), POINTER(c_uint32)]),
        "hrt_variance_defaults": (None, [POINTER(VarianceInfo)]),
        "hrt_accumulate_history_moments": (c_int32, [P, c_uint32]),
        "hrt_reproject_moments": (c_int32, [P, POINTER(ReprojectInfo), POINTER(View), P, POINTER(View), P]),
        "hrt_reproject_motion": (c_int32, [P, POINTER(ReprojectInfo), POINTER(MotionTables), POINTER(View), P,
                                           POINTER(View), P]),
        "hrt_reproject_motion_moments": (c_int32, [P, POINTER(ReprojectInfo), POINTER(MotionTables), POINTER(View), P,
                                                   POINTER(View), P]),
        "hrt_host_motion_between": (None, [POINTER(c_float), POINTER(c_float), POINTER(Motion)]),
        "hrt_fill_moments": (c_int32, [P, c_float, c_float]),
        "hrt_read_moments": (c_int32, [P, P, c_size_t]),
        "hrt_denoise_variance": (c_int32, [P, POINTER(VarianceInfo), P, c_uint32, P, c_size_t, P, c_size_t]),
        "hrt_denoise_variance_present": (c_int32, [P, POINTER(VarianceInfo), P, POINTER(PresentInfo), P, c_uint64,
                                                   POINTER(c_uint64)]),
        "hrt_upsample_defaults": (None, [POINTER(UpsampleInfo), c_uint32, c_uint32]),
        "hrt_upsample": (c_int32, [P, POINTER(UpsampleInfo), POINTER(DenoiseInfo), POINTER(VarianceInfo), P, P, c_uint32, P,
                                   c_size_t]),
        "hrt_upsample_present": (c_int32, [P, POINTER(UpsampleInfo), POINTER(DenoiseInfo), POINTER(VarianceInfo), P, P,
                                           POINTER(PresentInfo), P, c_uint64, POINTER(c_uint64)]),
        "hrt_order_after": (c_int32, [P, P]),
        "hrt_resolve_defaults": (None, [POINTER(ResolveInfo)]),
        "hrt_set_ray_grid": (c_int32, [P, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
        "hrt_history_phase": (None, [c_uint32, c_uint32, c_uint32, c_uint32, c_uint32, POINTER(c_float),
                                     POINTER(c_float)]),
        "hrt_accumulate_history_from": (c_int32, [P, P, POINTER(ResolveInfo), P, P]),
        "hrt_present_done": (c_int32, [P, c_uint64, POINTER(c_uint32)]),
        "hrt_present_wait": (c_int32, [P, c_uint64]),
        "hrt_debug_export_memory": (c_int32, [c_int32, c_uint64, POINTER(c_int32), POINTER(c_void_p),
                                              POINTER(c_uint64)]),
        "hrt_debug_unmap_memory": (c_int32, [P, c_uint64]),
        "hrt_debug_math_check": (c_int32, [c_int32, c_uint32, c_uint32, P]),
        "hrt_debug_math_check_rng": (c_int32, [c_int32, P]),
        "hrt_debug_band_flatten": (c_int32, [c_int32, P, P, c_uint32, P, P]),
        "hrt_debug_wq_protocol": (c_int32, [c_int32, c_uint32, P, P, P, P, P, P, P, P, P]),
        "hrt_debug_timeline": (c_int32, [c_void_p, P, c_uint32, P]),
        "hrt_debug_band_records": (c_int32, [c_void_p, P, c_uint64, P, c_uint64, P, c_uint64, P]),
        "hrt_debug_tile_costs": (c_int32, [c_void_p, P, c_uint32]),
        "hrt_debug_sky_units": (c_int32, [c_void_p, P]),
        "hrt_debug_tile_lists": (c_int32, [c_void_p, POINTER(PushConstants), c_uint32, P, c_uint64, P]),
        "hrt_debug_bvh_build": (c_int32, [P, c_uint32, P, c_uint32, c_uint32, P, P, c_uint64, P, c_uint64, P,
                                          c_uint64, P, c_uint64, P, c_uint64]),
        "hrt_debug_bvh_wq_nodes": (c_int64, [P, c_uint32, P, c_uint32, c_uint32, c_uint32, P, c_uint64]),
        "hrt_debug_bvh_wq_nodes_bfs": (c_int64, [P, c_uint32, P, c_uint32, c_uint32, c_uint32, P, c_uint64]),
        "hrt_debug_wq_l2_plan": (None, [c_uint32, c_uint32, c_uint32, c_int64, P]),
        "hrt_host_ray_grid": (c_uint32, [c_uint32, c_uint32, c_float, c_float, POINTER(c_float), POINTER(c_float),
                                         POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
        "hrt_set_option": (c_int32, [P, c_uint32, c_int64]),
        "hrt_stream": (c_void_p, [P]),
        "hrt_last_error": (c_char_p, [P]),
        "hrt_release_caches": (c_int32, [P]),
        "hrt_host_create_rays": (c_uint32, [c_uint32, c_uint32, c_float, c_float, POINTER(c_float), P,
                                            POINTER(c_float)]),
        "hrt_host_view_matrix": (None, [POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
        "hrt_host_transform_meshes": (c_int32, [c_uint32, P, P, P, P, P, P, c_uint32, P]),
        "hrt_obj_load": (c_int32, [c_char_p, POINTER(c_void_p)]),
        "hrt_obj_num_meshes": (c_uint32, [P]),
        "hrt_obj_mesh": (c_int32, [P, c_uint32, POINTER(c_char_p), POINTER(c_void_p), POINTER(c_uint32),
                                   POINTER(c_void_p), POINTER(c_uint32)]),
        "hrt_obj_free": (None, [P]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if path == LIB_PATH or path == DEBUG_LIB_PATH:
                raise  # the in-tree build must export the whole ABI (tests/test_abi.py)
            continue   # an older A/B build (HRT_LIB): calls of the missing entry point fail loudly
        fn.restype = res
        fn.argtypes = args
    _libs[debug] = lib
    return lib


def build_id() -> str:
    """hrt_build_id(): hash of the kernel sources + flags the loaded library was built from."""
    return load().hrt_build_id().decode()


def check(status: int, where: str, ctx=None, lib=None) -> None:
    if status != HRT_OK:
        detail = (lib or load()).hrt_last_error(ctx)
        raise HrtError(status, where, detail.decode() if detail else "")


def ptr(a: np.ndarray | None) -> c_void_p:
    if a is None or a.size == 0:
        return c_void_p(0)
    assert a.flags["C_CONTIGUOUS"]
    return c_void_p(a.ctypes.data)


def f3(v) -> ctypes.Array:
    return (c_float * 3)(*[float(np.float32(x)) for x in v])
