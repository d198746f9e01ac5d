"""Host side of the path: the Python mirror of RayTracePipeline (src/raytrace_pipeline.rs) and
DiffusePipeline (src/diffuse.rs) on top of the C ABI.  Host prep arithmetic (ray centres, view
matrix, mesh flattening) runs in the native library (hrt_host_*), the dispatches on the GPU.

Mapping to the reference:
  RayTracerSettings        src/raytracing_app.rs:17-29
  RayTracePipeline.__init__ src/raytrace_pipeline.rs:51-97   (-> hrt_create + hrt_set_scene)
  RayTracePipeline.compute  src/raytrace_pipeline.rs:162-187 (-> hrt_trace, init = 0)
  RayTracePipeline.init     src/raytrace_pipeline.rs:190-213 (-> hrt_trace, init = 1)
  RayTracePipeline.push_constants  dispatch :216-266 (124-byte block :243-257)
  DiffusePipeline.next_frame       src/diffuse.rs:73-101 (-> hrt_accumulate)
  RenderPassOverFrame.render       src/texture_draw_pipeline.rs:96-157 (-> hrt_present)
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .scene import Camera, RayTracingMesh, Sphere, as_material, get_null_mesh, get_null_sphere


@dataclass
class RayTracerSettings:
    """src/raytracing_app.rs:17-29."""
    num_samples: int
    max_bounces: int
    use_environment_lighting: bool
    sample_jitter: Optional[float] = None
    sphere_data: List[Sphere] = field(default_factory=list)
    mesh_data: List[RayTracingMesh] = field(default_factory=list)
    camera_focal_length: float = 1.0
    viewport_height: float = 2.0
    up: Sequence[float] = (0.0, 1.0, 0.0)


# ---- host prep (native) ---------------------------------------------------------------------

def create_rays(image_size, camera_focal_length, viewport_height, up):
    """create_ray_subbuffer, src/raytrace_pipeline.rs:289-338 -> (rays[W*H], num_rays, default_jitter)."""
    lib = _lib.load()
    w, h = int(image_size[0]), int(image_size[1])
    rays = np.zeros(max(w * h, 1), dtype=_lib.RAY_DTYPE)
    jit = ctypes.c_float()
    n = lib.hrt_host_create_rays(w, h, float(np.float32(camera_focal_length)), float(np.float32(viewport_height)),
                                 _lib.f3(up), _lib.ptr(rays), ctypes.byref(jit))
    return rays, int(n), float(jit.value)


def view_matrix(direction, up) -> np.ndarray:
    """get_view_matrix, src/raytrace_pipeline.rs:269-285 -> column-major mat4 as float32[16]."""
    lib = _lib.load()
    out = (ctypes.c_float * 16)()
    lib.hrt_host_view_matrix(_lib.f3(direction), _lib.f3(up), out)
    return np.frombuffer(out, dtype=np.float32).copy()


def transform_meshes(meshes: List[RayTracingMesh]):
    """transform_meshes, src/raytrace_pipeline.rs:377-428 -> (triangles, mesh records)."""
    lib = _lib.load()
    n = len(meshes)
    pos = [np.ascontiguousarray(m.mesh.positions, np.float32) for m in meshes]
    idx = [np.ascontiguousarray(m.mesh.indices, np.uint32) for m in meshes]
    mats = np.array([as_material(m.material) for m in meshes], dtype=_lib.MATERIAL_DTYPE)
    ntri = sum(int(i.size) // 3 for i in idx)
    tris = np.zeros(max(ntri, 1), dtype=_lib.TRIANGLE_DTYPE)
    recs = np.zeros(max(n, 1), dtype=_lib.MESH_DTYPE)
    pos_ptrs = (ctypes.c_void_p * n)(*[p.ctypes.data for p in pos])
    idx_ptrs = (ctypes.c_void_p * n)(*[i.ctypes.data if i.size else 0 for i in idx])
    nv = (ctypes.c_uint32 * n)(*[p.shape[0] for p in pos])
    ni = (ctypes.c_uint32 * n)(*[i.size for i in idx])
    st = lib.hrt_host_transform_meshes(n, pos_ptrs, nv, idx_ptrs, ni, _lib.ptr(mats), _lib.ptr(tris), ntri,
                                       _lib.ptr(recs))
    _lib.check(st, "hrt_host_transform_meshes")
    return tris[:ntri], recs[:n]


def sphere_records(spheres: List[Sphere]) -> np.ndarray:
    """create_sphere_subbuffer, src/raytrace_pipeline.rs:342-360."""
    if not spheres:
        return np.zeros(0, dtype=_lib.SPHERE_DTYPE)
    return np.array([s.record() for s in spheres], dtype=_lib.SPHERE_DTYPE)


def ray_grid(image_size, camera_focal_length, viewport_height, up):
    """hrt_host_ray_grid: (first, dx, dy, default jitter) of an image's ray centres, ray (x, y) = (first + dx * x)
    + dy * y; the three vectors as float32 arrays of 3."""
    first, dx, dy = ((ctypes.c_float * 3)() for _ in range(3))
    jit = ctypes.c_float()
    _lib.load().hrt_host_ray_grid(int(image_size[0]), int(image_size[1]), float(np.float32(camera_focal_length)),
                                  float(np.float32(viewport_height)), _lib.f3(up), first, dx, dy, ctypes.byref(jit))
    return (np.array(first[:], np.float32), np.array(dx[:], np.float32), np.array(dy[:], np.float32), jit.value)


def motion_between(prev_pose, cur_pose) -> _lib.Motion:
    """hrt_host_motion_between: the ``_lib.Motion`` record of an object whose object-to-world pose -- 12 floats, a
    column-major 3x4 [R | t] with R a rotation -- was ``prev_pose`` in the previous frame and is ``cur_pose`` now."""
    a = np.ascontiguousarray(prev_pose, dtype=np.float32).reshape(12)
    b = np.ascontiguousarray(cur_pose, dtype=np.float32).reshape(12)
    out = _lib.Motion()
    fp = ctypes.POINTER(ctypes.c_float)
    _lib.load().hrt_host_motion_between(a.ctypes.data_as(fp), b.ctypes.data_as(fp), ctypes.byref(out))
    return out


def shifted_first(first, dx, dy, ox, oy) -> np.ndarray:
    """The first ray centre of a grid shifted by (ox, oy) pixels: (first + ox * dx) + oy * dy, every operation in
    binary32 -- what hrt_set_ray_grid takes as ``first`` for frame k's ``history_phase`` offset."""
    first, dx, dy = (np.asarray(v, np.float32)[:3] for v in (first, dx, dy))
    ox, oy = np.float32(ox), np.float32(oy)
    return ((first + ox * dx).astype(np.float32) + (oy * dy).astype(np.float32)).astype(np.float32)


def history_phase(source_size, target_size, k: int):
    """hrt_history_phase: the sub-pixel offset (ox, oy) of frame k of a source_size grid that feeds a target_size
    history through ``HrtContext.accumulate_history_from``."""
    ox, oy = ctypes.c_float(), ctypes.c_float()
    _lib.load().hrt_history_phase(int(source_size[0]), int(target_size[0]), int(source_size[1]), int(target_size[1]),
                                  int(k) & 0xFFFFFFFF, ctypes.byref(ox), ctypes.byref(oy))
    return ox.value, oy.value


class View:
    """hrt_view of a camera: its position and view matrix as ``RayTracePipeline.push_constants`` writes them,
    and the affine grid of the ray centres (hrt_host_ray_grid) of an image of ``image_size`` under
    ``settings`` (anything with camera_focal_length, viewport_height and up).  ``record`` is the
    _lib.View that hrt_reproject takes.  ``offset`` = (ox, oy): the view of a grid shifted by that many pixels
    (``shifted_first``), as ``HrtContext.shift_ray_grid`` sets it."""

    def __init__(self, camera: Camera, image_size, settings, offset=None):
        lib = _lib.load()
        first, dx, dy = ((ctypes.c_float * 3)() for _ in range(3))
        lib.hrt_host_ray_grid(int(image_size[0]), int(image_size[1]), float(np.float32(settings.camera_focal_length)),
                              float(np.float32(settings.viewport_height)), _lib.f3(settings.up), first, dx, dy, None)
        if offset is not None:
            first = shifted_first(first[:], dx[:], dy[:], offset[0], offset[1])
        rec = _lib.View()
        pos = np.asarray(camera.position, np.float32)
        rec.cam_pos[:] = [float(pos[0]), float(pos[1]), float(pos[2]), 1.0]
        rec.cam_alignment_mat[:] = [float(v) for v in view_matrix(camera.direction, camera.up)]
        for dst, src in ((rec.grid_first, first), (rec.grid_dx, dx), (rec.grid_dy, dy)):
            dst[:] = [float(src[0]), float(src[1]), float(src[2]), 0.0]
        self.record = rec


# ---- the device context (one hrt_context = the trace image + the accumulated image) ------------

class HrtContext:
    """Owner of one hrt_context.  ``partition`` = (row_tile, part_index, part_count) selects the
    interleaved row tiles this context renders (multi-GPU).  ``debug=True`` binds
    libhip_raytrace_debug.so (diagnostics-only options)."""

    def __init__(self, image_size, device: int = -1, mode: int = _lib.MODE_RGBA8, partition=None,
                 debug: bool = False):
        self.lib = _lib.load(debug)
        info = _lib.CreateInfo()
        info.width, info.height = int(image_size[0]), int(image_size[1])
        info.device = int(device)
        info.mode = int(mode)
        if partition is not None:
            info.row_tile, info.part_index, info.part_count = (int(v) for v in partition)
        else:
            info.row_tile, info.part_index, info.part_count = 0, 0, 1
        h = ctypes.c_void_p()
        _lib.check(self.lib.hrt_create(ctypes.byref(info), ctypes.byref(h)), "hrt_create", None, self.lib)
        self.handle = h
        lay = _lib.Layout()
        _lib.check(self.lib.hrt_get_layout(self.handle, ctypes.byref(lay)), "hrt_get_layout", self.handle, self.lib)
        self.width, self.height = lay.width, lay.height
        self.local_rows, self.row_tile = lay.local_rows, lay.row_tile
        self.part_index, self.part_count, self.mode = lay.part_index, lay.part_count, lay.mode

    def close(self):
        if getattr(self, "handle", None):
            self.lib.hrt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st, where):
        _lib.check(st, where, self.handle, self.lib)

    def set_scene(self, rays, spheres, tris, meshes):
        """rays=None keeps the context's rays (hrt_generate_rays or an earlier set_scene)."""
        n_rays = 0 if rays is None else len(rays)
        self._check(self.lib.hrt_set_scene(self.handle, None if rays is None else _lib.ptr(rays), n_rays,
                                           _lib.ptr(spheres), len(spheres), _lib.ptr(tris), len(tris),
                                           _lib.ptr(meshes), len(meshes)),
                    "hrt_set_scene")

    def generate_rays(self, camera_focal_length: float, viewport_height: float, up) -> float:
        """Ray centres on the device (hrt_generate_rays); returns the default jitter."""
        u = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in up])
        jit = ctypes.c_float()
        self._check(self.lib.hrt_generate_rays(self.handle, float(np.float32(camera_focal_length)),
                                               float(np.float32(viewport_height)), u, ctypes.byref(jit)),
                    "hrt_generate_rays")
        return jit.value

    def import_external(self, fd: int, size: int, offset: int, nbytes: int) -> int:
        """hrt_import_external_memory: device pointer (int) to [offset, offset + nbytes) of the fd."""
        ptr = ctypes.c_void_p()
        self._check(self.lib.hrt_import_external_memory(self.handle, int(fd), int(size), int(offset), int(nbytes),
                                                        ctypes.byref(ptr)), "hrt_import_external_memory")
        return int(ptr.value)

    def release_external(self, dev_ptr: int):
        self._check(self.lib.hrt_release_external_memory(self.handle, ctypes.c_void_p(dev_ptr)),
                    "hrt_release_external_memory")

    def read_rays(self) -> np.ndarray:
        out = np.empty(self.width * self.height, dtype=_lib.RAY_DTYPE)
        self._check(self.lib.hrt_read_rays(self.handle, _lib.ptr(out), len(out)), "hrt_read_rays")
        return out

    def trace(self, pc: _lib.PushConstants):
        self._check(self.lib.hrt_trace(self.handle, ctypes.byref(pc)), "hrt_trace")

    def accumulate(self, frame: int):
        self._check(self.lib.hrt_accumulate(self.handle, int(frame) & 0xFFFFFFFF), "hrt_accumulate")

    def compute_n(self, pc: _lib.PushConstants, n: int):
        """hrt_compute_n: n x (trace with rng_offset = pc.rng_offset + k, accumulate(that k))."""
        self._check(self.lib.hrt_compute_n(self.handle, ctypes.byref(pc), int(n)), "hrt_compute_n")

    def compute_until(self, pc: _lib.PushConstants, max_frames: int, max_changed_pixels: int = _lib.RULE_ANY,
                      max_delta: int = _lib.RULE_ANY, quiet_frames: int = 1):
        """hrt_compute_until: compute_n stopped after the first run of quiet_frames consecutive quiet frames
        (a frame is quiet when its fold record has changed_pixels <= max_changed_pixels and max_delta <=
        max_delta).  Blocking.  Returns (frames_done, settled)."""
        rule = _lib.SettleRule(int(max_changed_pixels), int(max_delta), int(quiet_frames), 0)
        done, settled = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.hrt_compute_until(self.handle, ctypes.byref(pc), int(max_frames), ctypes.byref(rule),
                                               ctypes.byref(done), ctypes.byref(settled)), "hrt_compute_until")
        return done.value, bool(settled.value)

    def fold_records(self, cap: int = _lib.FOLD_RECORD_RING, with_total: bool = False):
        """hrt_get_fold_records: the newest min(cap, available) records (OPT_FOLD_RECORDS = 1), oldest first,
        as a structured array (_lib.FOLD_RECORD_DTYPE); with_total=True returns (records, total appended
        since the option was set)."""
        out = np.zeros(max(int(cap), 0), dtype=_lib.FOLD_RECORD_DTYPE)
        n, total = ctypes.c_uint32(), ctypes.c_uint64()
        self._check(self.lib.hrt_get_fold_records(self.handle, _lib.ptr(out), len(out), ctypes.byref(n),
                                                  ctypes.byref(total)), "hrt_get_fold_records")
        recs = out[:n.value].copy()
        return (recs, total.value) if with_total else recs

    def synchronize(self):
        self._check(self.lib.hrt_synchronize(self.handle), "hrt_synchronize")

    def set_option(self, key: int, value: int):
        self._check(self.lib.hrt_set_option(self.handle, key, value), "hrt_set_option")

    def stats(self) -> _lib.Stats:
        s = _lib.Stats()
        self._check(self.lib.hrt_get_stats(self.handle, ctypes.byref(s)), "hrt_get_stats")
        return s

    def diagnostics(self) -> dict:
        """Cull diagnostics (needs set_option(OPT_COUNTERS, 2) before the traces)."""
        out = np.zeros(len(_lib.DIAG_NAMES), np.uint64)
        self._check(self.lib.hrt_get_diagnostics(self.handle, _lib.ptr(out), len(out)), "hrt_get_diagnostics")
        return dict(zip(_lib.DIAG_NAMES, (int(v) for v in out)))

    def tile_profile(self) -> np.ndarray:
        """Per 8x8 tile of the last trace, (ceil(local_rows/8), ceil(W/8), 4): shader clocks, bounce
        iterations, bounce survivor tests, bounce clocks (needs OPT_COUNTERS=2)."""
        ty, tx = (self.local_rows + 7) // 8, (self.width + 7) // 8
        out = np.zeros(ty * tx * 4, np.uint64)
        self._check(self.lib.hrt_get_tile_profile(self.handle, _lib.ptr(out), len(out)), "hrt_get_tile_profile")
        return out.reshape(ty, tx, 4)

    def scene_info(self) -> dict:
        """What the last set_scene built for the BVH kernel (hrt_get_scene_info)."""
        out = np.zeros(len(_lib.SCENE_INFO_NAMES), np.uint32)
        self._check(self.lib.hrt_get_scene_info(self.handle, _lib.ptr(out), len(out)), "hrt_get_scene_info")
        return dict(zip(_lib.SCENE_INFO_NAMES, (int(v) for v in out)))

    def reset_stats(self):
        self._check(self.lib.hrt_reset_stats(self.handle), "hrt_reset_stats")

    def read(self, image_id: int, fmt: int = _lib.FMT_RGBA8) -> np.ndarray:
        """Local rows of an image: uint8 (local_rows, W, 4) or float32 (local_rows, W, 4) -- this
        context's own rows even when it is joined to a communicator (HRT_IMG_LOCAL: never the
        collective gather; read_frame is the gathered frame)."""
        dt = np.uint8 if fmt == _lib.FMT_RGBA8 else np.float32
        out = np.empty((self.local_rows, self.width, 4), dtype=dt)
        self._check(self.lib.hrt_read_image(self.handle, image_id | _lib.IMG_LOCAL, fmt, _lib.ptr(out), out.nbytes),
                    "hrt_read_image")
        return out

    def load_accumulator(self, img: np.ndarray):
        """Checkpoint / resume: restore the accumulated image from an earlier read(IMG_ACCUM) in the
        context's own format (hrt_load_accumulator)."""
        fmt = _lib.FMT_RGBA8 if self.mode == _lib.MODE_RGBA8 else _lib.FMT_RGBA32F
        img = np.ascontiguousarray(img)
        self._check(self.lib.hrt_load_accumulator(self.handle, fmt, _lib.ptr(img), img.nbytes), "hrt_load_accumulator")

    def read_into(self, image_id: int, fmt: int, dst_ptr: int, nbytes: int):
        """Copy into caller memory (host or device pointer, e.g. a torch tensor's data_ptr())."""
        self._check(self.lib.hrt_read_image(self.handle, image_id, fmt, ctypes.c_void_p(dst_ptr), nbytes),
                    "hrt_read_image")

    # ---- the present pass (hrt_present) ----

    def _present_info(self, image_id, width, height, pitch, fmt) -> _lib.PresentInfo:
        width, height = int(width), int(height)
        return _lib.PresentInfo(int(image_id), int(fmt), width, height, width * 4 if pitch is None else int(pitch), 0)

    def present(self, image_id: int, dst_ptr: int, nbytes: int, width: int, height: int, pitch: Optional[int] = None,
                fmt: int = _lib.PRESENT_B8G8R8A8) -> int:
        """hrt_present: enqueue the image as the reference's flipped, nearest-sampled quad over the
        width x height target at device pointer dst_ptr (rows pitch bytes apart, default width * 4) and
        return its ticket without waiting (at most 8 in flight).  On the root (part 0) of a comm_init_all
        group the image is the group's gathered full frame (width x height, not local_rows); the other
        members, a comm_init-joined context and a partitioned context with no communicator are rejected."""
        info, t = self._present_info(image_id, width, height, pitch, fmt), ctypes.c_uint64()
        self._check(self.lib.hrt_present(self.handle, ctypes.byref(info), ctypes.c_void_p(dst_ptr), int(nbytes),
                                         ctypes.byref(t)), "hrt_present")
        return t.value

    def accumulate_present(self, frame: int, dst_ptr: int, nbytes: int, width: int, height: int,
                           pitch: Optional[int] = None, fmt: int = _lib.PRESENT_B8G8R8A8) -> int:
        """hrt_accumulate_present: accumulate(frame) and present(IMG_ACCUM, ...) in one call (one kernel
        when the target has the image's size and combines are not deferred); returns the ticket.  On the
        root of a comm_init_all group: accumulate(frame) on every member in part order, then the gathered
        present."""
        info, t = self._present_info(_lib.IMG_ACCUM, width, height, pitch, fmt), ctypes.c_uint64()
        self._check(self.lib.hrt_accumulate_present(self.handle, int(frame) & 0xFFFFFFFF, ctypes.byref(info),
                                                    ctypes.c_void_p(dst_ptr), int(nbytes), ctypes.byref(t)),
                    "hrt_accumulate_present")
        return t.value

    def present_done(self, ticket: int) -> bool:
        """Whether the present pass of `ticket` has finished (a poll)."""
        done = ctypes.c_uint32()
        self._check(self.lib.hrt_present_done(self.handle, int(ticket), ctypes.byref(done)), "hrt_present_done")
        return bool(done.value)

    def present_wait(self, ticket: int):
        """Block until the present pass of `ticket` has finished."""
        self._check(self.lib.hrt_present_wait(self.handle, int(ticket)), "hrt_present_wait")

    # ---- the denoise pass (hrt_denoise, hrt_denoise_present) ----

    def denoise_info(self, image_id: int = _lib.IMG_ACCUM, iterations: Optional[int] = None,
                     method: int = _lib.DENOISE_AUTO, sigma_colour: Optional[float] = None,
                     sigma_normal: Optional[float] = None, sigma_depth: Optional[float] = None) -> _lib.DenoiseInfo:
        """hrt_denoise_defaults with the given fields replaced (None: the default)."""
        info = _lib.DenoiseInfo()
        self.lib.hrt_denoise_defaults(ctypes.byref(info))
        info.image_id, info.method = int(image_id), int(method)
        if iterations is not None:
            info.iterations = int(iterations)
        for name, v in (("sigma_colour", sigma_colour), ("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth)):
            if v is not None:
                setattr(info, name, float(v))
        return info

    def denoise_into(self, dst_ptr: int, nbytes: int, fmt: int = _lib.FMT_RGBA8, guide_ptr: Optional[int] = None,
                     info: Optional[_lib.DenoiseInfo] = None, **fields):
        """hrt_denoise into caller memory (host or device pointer): the guided a-trous filter
        of image ``image_id`` as local_rows x W texels of fmt.  guide_ptr: None for the colour-only filter, else
        a 16-byte aligned device pointer to W x H hrt_hit records (``intersect_primary_into`` of the whole
        image).  ``info`` or the fields of ``denoise_info``.  Blocking."""
        info = info if info is not None else self.denoise_info(**fields)
        self._check(self.lib.hrt_denoise(self.handle, ctypes.byref(info), ctypes.c_void_p(guide_ptr or 0), int(fmt),
                                         ctypes.c_void_p(dst_ptr), int(nbytes)), "hrt_denoise")

    def denoise(self, fmt: int = _lib.FMT_RGBA8, guide_ptr: Optional[int] = None,
                info: Optional[_lib.DenoiseInfo] = None, **fields) -> np.ndarray:
        """hrt_denoise: the filtered image as uint8 or float32 (local_rows, W, 4)."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.uint8 if fmt == _lib.FMT_RGBA8 else np.float32)
        self.denoise_into(out.ctypes.data, out.nbytes, fmt, guide_ptr, info, **fields)
        return out

    def denoise_present(self, dst_ptr: int, nbytes: int, width: int, height: int, pitch: Optional[int] = None,
                        fmt: int = _lib.PRESENT_B8G8R8A8, guide_ptr: Optional[int] = None,
                        info: Optional[_lib.DenoiseInfo] = None, **fields) -> int:
        """hrt_denoise_present: the filter, then ``present`` of the filtered image (same target rules, same
        ticket sequence); returns the ticket without waiting."""
        info = info if info is not None else self.denoise_info(**fields)
        target, t = self._present_info(info.image_id, width, height, pitch, fmt), ctypes.c_uint64()
        self._check(self.lib.hrt_denoise_present(self.handle, ctypes.byref(info), ctypes.c_void_p(guide_ptr or 0),
                                                 ctypes.byref(target), ctypes.c_void_p(dst_ptr), int(nbytes),
                                                 ctypes.byref(t)), "hrt_denoise_present")
        return t.value

    # ---- guided upsampling (hrt_upsample, hrt_upsample_present, hrt_order_after) ----

    def upsample_info(self, width: int, height: int, image_id: int = _lib.IMG_ACCUM, footprint: Optional[int] = None,
                      sigma_normal: Optional[float] = None, sigma_depth: Optional[float] = None) -> _lib.UpsampleInfo:
        """hrt_upsample_defaults for a width x height result with the given fields replaced (None: the default)."""
        info = _lib.UpsampleInfo()
        self.lib.hrt_upsample_defaults(ctypes.byref(info), int(width), int(height))
        info.image_id = int(image_id)
        if footprint is not None:
            info.footprint = int(footprint)
        for name, v in (("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth)):
            if v is not None:
                setattr(info, name, float(v))
        return info

    def upsample_into(self, dst_ptr: int, nbytes: int, width: int, height: int, low_hits_ptr: int, high_hits_ptr: int,
                      fmt: int = _lib.FMT_RGBA8, denoise: Optional[_lib.DenoiseInfo] = None,
                      variance: Optional[_lib.VarianceInfo] = None, info: Optional[_lib.UpsampleInfo] = None, **fields):
        """hrt_upsample into caller memory (host or device pointer): this context's image at width x height, a
        joint-bilateral reconstruction guided by low_hits_ptr (this context's W x H hrt_hit records)
        and high_hits_ptr (width x height records of the same view), both 16-byte aligned device pointers.
        ``denoise`` or ``variance`` (at most one): that filter runs over the low image first.  ``info`` or the
        fields of ``upsample_info``.  Blocking."""
        info = info if info is not None else self.upsample_info(width, height, **fields)
        self._check(self.lib.hrt_upsample(self.handle, ctypes.byref(info),
                                          ctypes.byref(denoise) if denoise is not None else None,
                                          ctypes.byref(variance) if variance is not None else None,
                                          ctypes.c_void_p(low_hits_ptr or 0), ctypes.c_void_p(high_hits_ptr or 0), int(fmt),
                                          ctypes.c_void_p(dst_ptr), int(nbytes)), "hrt_upsample")

    def upsample(self, width: int, height: int, low_hits_ptr: int, high_hits_ptr: int, fmt: int = _lib.FMT_RGBA8,
                 denoise: Optional[_lib.DenoiseInfo] = None, variance: Optional[_lib.VarianceInfo] = None,
                 info: Optional[_lib.UpsampleInfo] = None, **fields) -> np.ndarray:
        """hrt_upsample: the reconstructed image as uint8 or float32 (height, width, 4)."""
        out = np.empty((int(height), int(width), 4), dtype=np.uint8 if fmt == _lib.FMT_RGBA8 else np.float32)
        self.upsample_into(out.ctypes.data, out.nbytes, width, height, low_hits_ptr, high_hits_ptr, fmt, denoise, variance,
                           info, **fields)
        return out

    def upsample_present(self, dst_ptr: int, nbytes: int, width: int, height: int, low_hits_ptr: int, high_hits_ptr: int,
                         pitch: Optional[int] = None, fmt: int = _lib.PRESENT_B8G8R8A8,
                         denoise: Optional[_lib.DenoiseInfo] = None, variance: Optional[_lib.VarianceInfo] = None,
                         info: Optional[_lib.UpsampleInfo] = None, **fields) -> int:
        """hrt_upsample_present: the reconstruction written straight into the width x height target as ``present``
        writes an image of the target's size (same target rules, same ticket sequence); returns the ticket without
        waiting."""
        info = info if info is not None else self.upsample_info(width, height, **fields)
        target, t = self._present_info(info.image_id, width, height, pitch, fmt), ctypes.c_uint64()
        self._check(self.lib.hrt_upsample_present(self.handle, ctypes.byref(info),
                                                  ctypes.byref(denoise) if denoise is not None else None,
                                                  ctypes.byref(variance) if variance is not None else None,
                                                  ctypes.c_void_p(low_hits_ptr or 0), ctypes.c_void_p(high_hits_ptr or 0),
                                                  ctypes.byref(target), ctypes.c_void_p(dst_ptr), int(nbytes),
                                                  ctypes.byref(t)), "hrt_upsample_present")
        return t.value

    def order_after(self, producer: "HrtContext"):
        """hrt_order_after: work issued on this context from now on follows everything issued so far on
        ``producer``'s stream (an event and a stream wait; no host wait).  Both must be on one device."""
        self._check(self.lib.hrt_order_after(self.handle, producer.handle), "hrt_order_after")

    # ---- temporal upsampling (hrt_set_ray_grid, hrt_accumulate_history_from) ----

    def set_ray_grid(self, first, dx, dy):
        """hrt_set_ray_grid: the ray centres become (first + dx * x) + dy * y, written on the device in stream
        order -- no host wait.  The grid is remembered as the base of ``shift_ray_grid``."""
        self._check(self.lib.hrt_set_ray_grid(self.handle, _lib.f3(first), _lib.f3(dx), _lib.f3(dy)), "hrt_set_ray_grid")
        self.base_grid = tuple(np.asarray(v, np.float32)[:3].copy() for v in (first, dx, dy))

    def shift_ray_grid(self, ox: float, oy: float, grid=None):
        """The ray centres of ``grid`` = (first, dx, dy) shifted by (ox, oy) pixels (``shifted_first``); grid=None:
        the grid of the last ``set_ray_grid``.  Typically (ox, oy) = ``history_phase(...)`` of the frame."""
        grid = grid if grid is not None else getattr(self, "base_grid", None)
        if grid is None:
            raise ValueError("no base grid: pass grid=(first, dx, dy) or call set_ray_grid first")
        first, dx, dy = grid[:3]
        self._check(self.lib.hrt_set_ray_grid(self.handle, _lib.f3(shifted_first(first, dx, dy, ox, oy)), _lib.f3(dx),
                                              _lib.f3(dy)), "hrt_set_ray_grid")

    def resolve_info(self, offset=(0.0, 0.0), max_history: Optional[int] = None, moments: bool = False,
                     fill: Optional[bool] = None) -> _lib.ResolveInfo:
        """hrt_resolve_defaults with the given fields replaced (None: the default)."""
        info = _lib.ResolveInfo()
        self.lib.hrt_resolve_defaults(ctypes.byref(info))
        info.offset_x, info.offset_y = float(np.float32(offset[0])), float(np.float32(offset[1]))
        if max_history is not None:
            info.max_history = int(max_history)
        if fill is not None:
            info.flags = (info.flags & ~_lib.RESOLVE_FILL) | (_lib.RESOLVE_FILL if fill else 0)
        if moments:
            info.flags |= _lib.RESOLVE_MOMENTS
        return info

    def accumulate_history_from(self, source: "HrtContext", offset=(0.0, 0.0), max_history: Optional[int] = None,
                                moments: bool = False, fill: Optional[bool] = None, source_hits_ptr: Optional[int] = None,
                                hits_ptr: Optional[int] = None, info: Optional[_lib.ResolveInfo] = None):
        """hrt_accumulate_history_from: ``source``'s trace image, sampled on a grid shifted by ``offset`` pixels of
        its own, folded into this context's history -- each texel into the pixel its sample landed in.  The two
        hit pointers (device memory, both or neither) restrict it to pixels whose first hits share a surface.
        Non-blocking."""
        info = info if info is not None else self.resolve_info(offset, max_history, moments, fill)
        self._check(self.lib.hrt_accumulate_history_from(self.handle, source.handle, ctypes.byref(info),
                                                         ctypes.c_void_p(source_hits_ptr or 0),
                                                         ctypes.c_void_p(hits_ptr or 0)),
                    "hrt_accumulate_history_from")

    # ---- temporal history (hrt_reproject, hrt_accumulate_history, hrt_fill_history, hrt_read_history) ----

    def reproject_info(self, filter: Optional[int] = None, depth_tolerance: Optional[float] = None,  # noqa: A002
                       min_normal_dot: Optional[float] = None) -> _lib.ReprojectInfo:
        """hrt_reproject_defaults with the given fields replaced (None: the default)."""
        info = _lib.ReprojectInfo()
        self.lib.hrt_reproject_defaults(ctypes.byref(info))
        if filter is not None:
            info.filter = int(filter)
        if depth_tolerance is not None:
            info.depth_tolerance = float(depth_tolerance)
        if min_normal_dot is not None:
            info.min_normal_dot = float(min_normal_dot)
        return info

    def reproject(self, prev: "View", prev_hits_ptr: int, cur: "View", cur_hits_ptr: int,
                  info: Optional[_lib.ReprojectInfo] = None, **fields) -> None:
        """hrt_reproject: the accumulator and the count image of view ``prev`` become those of view ``cur``
        (DESIGN.md S15).  The hit pointers are 16-byte aligned device pointers to W x H hrt_hit records
        (``intersect_primary_into`` of the whole image under each view).  ``info`` or the fields of
        ``reproject_info``.  Only enqueues: keep the hit arrays unchanged until the pass has run."""
        info = info if info is not None else self.reproject_info(**fields)
        self._check(self.lib.hrt_reproject(self.handle, ctypes.byref(info), ctypes.byref(prev.record),
                                           ctypes.c_void_p(prev_hits_ptr), ctypes.byref(cur.record),
                                           ctypes.c_void_p(cur_hits_ptr)), "hrt_reproject")

    def accumulate_history(self, max_history: int) -> None:
        """hrt_accumulate_history: the trace image folded into the accumulator with every pixel's own frame
        count, which then grows by one up to max_history (1 .. 2^24)."""
        self._check(self.lib.hrt_accumulate_history(self.handle, int(max_history)), "hrt_accumulate_history")

    def fill_history(self, count: int) -> None:
        """hrt_fill_history: every pixel's count = count (0: no history)."""
        self._check(self.lib.hrt_fill_history(self.handle, int(count)), "hrt_fill_history")

    def read_history_into(self, dst_ptr: int, nbytes: int) -> None:
        """hrt_read_history into caller memory (host or device pointer).  Blocking."""
        self._check(self.lib.hrt_read_history(self.handle, ctypes.c_void_p(dst_ptr), int(nbytes)), "hrt_read_history")

    def read_history(self) -> np.ndarray:
        """hrt_read_history: the count image as uint32 (local_rows, W)."""
        out = np.empty((self.local_rows, self.width), dtype=np.uint32)
        self.read_history_into(out.ctypes.data, out.nbytes)
        return out

    # ---- adaptive refinement (hrt_refine_select, hrt_refine, hrt_refine_until) ----

    @property
    def mask_words(self) -> int:
        """The uint32 words of a selection mask: one bit per pixel, pixel i = x + y W in bit i & 31 of word i >> 5."""
        return (self.local_rows * self.width + 31) // 32

    def refine_rule(self, min_history: Optional[int] = None, max_count: Optional[int] = None,
                    radius: Optional[int] = None, tolerance: Optional[float] = None,
                    luminance_floor: Optional[float] = None) -> _lib.RefineRule:
        """hrt_refine_defaults with the given fields replaced (None: the default)."""
        rule = _lib.RefineRule()
        self.lib.hrt_refine_defaults(ctypes.byref(rule))
        for name, v in (("min_history", min_history), ("max_count", max_count), ("radius", radius)):
            if v is not None:
                setattr(rule, name, int(v))
        for name, v in (("tolerance", tolerance), ("luminance_floor", luminance_floor)):
            if v is not None:
                setattr(rule, name, float(v))
        return rule

    def refine_select_into(self, mask_ptr: int, guide_ptr: Optional[int] = None, want_count: bool = True,
                           rule: Optional[_lib.RefineRule] = None, **fields) -> Optional[int]:
        """hrt_refine_select into caller memory (host or 4-byte aligned device pointer, ``mask_words`` words): the
        pixels whose pooled standard error is above the rule's tolerance.  guide_ptr as
        ``denoise_into`` takes it.  Returns the number selected; want_count False with a device mask only enqueues."""
        rule = rule if rule is not None else self.refine_rule(**fields)
        n = ctypes.c_uint64()
        self._check(self.lib.hrt_refine_select(self.handle, ctypes.byref(rule), ctypes.c_void_p(guide_ptr or 0),
                                               ctypes.c_void_p(mask_ptr), ctypes.byref(n) if want_count else None),
                    "hrt_refine_select")
        return n.value if want_count else None

    def refine_select(self, guide_ptr: Optional[int] = None, rule: Optional[_lib.RefineRule] = None, **fields):
        """hrt_refine_select: (mask as uint32 (mask_words,), the number of selected pixels)."""
        mask = np.empty(self.mask_words, dtype=np.uint32)
        n = self.refine_select_into(mask.ctypes.data, guide_ptr, True, rule, **fields)
        return mask, n

    def refine(self, pc: _lib.PushConstants, mask, max_history: int, method: int = _lib.REFINE_AUTO,
               query_method: int = 0, moments: bool = True, want_stats: bool = True) -> Optional[_lib.RefineStats]:
        """hrt_refine: one new sample of frame ``pc`` for every pixel set in ``mask`` (a uint32 array in host memory or
        an int device pointer), folded as ``accumulate_history[_moments]`` folds it; the other pixels keep their
        bytes.  Blocking."""
        if isinstance(mask, np.ndarray):
            mask = np.ascontiguousarray(mask, dtype=np.uint32)
            assert mask.size >= self.mask_words
            ptr = mask.ctypes.data
        else:
            ptr = int(mask)
        st = _lib.RefineStats()
        self._check(self.lib.hrt_refine(self.handle, ctypes.byref(pc), ctypes.c_void_p(ptr), int(max_history), int(method),
                                        int(query_method), _lib.REFINE_MOMENTS if moments else 0,
                                        ctypes.byref(st) if want_stats else None), "hrt_refine")
        return st if want_stats else None

    def refine_until(self, pc: _lib.PushConstants, max_history: int, max_passes: int, guide_ptr: Optional[int] = None,
                     method: int = _lib.REFINE_AUTO, rule: Optional[_lib.RefineRule] = None, **fields):
        """hrt_refine_until: select-and-refine passes with rng_offset pc.rng_offset, + 1, ... until nothing is
        selected or max_passes have run.  Returns (passes done, pixel-frames traced, settled)."""
        rule = rule if rule is not None else self.refine_rule(**fields)
        passes, frames, settled = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self.lib.hrt_refine_until(self.handle, ctypes.byref(pc), ctypes.byref(rule),
                                              ctypes.c_void_p(guide_ptr or 0), int(max_history), int(max_passes),
                                              int(method), _lib.REFINE_MOMENTS, ctypes.byref(passes), ctypes.byref(frames),
                                              ctypes.byref(settled)), "hrt_refine_until")
        return passes.value, frames.value, bool(settled.value)

    def refine_tiles(self, pc: _lib.PushConstants, mask, max_history: int, frames: int = 1, moments: bool = True,
                     want_stats: bool = True) -> Optional[_lib.RefineTilesStats]:
        """hrt_refine_tiles: ``frames`` new frames (rng_offset pc.rng_offset, + 1, ...) for every pixel set in
        ``mask`` (a uint32 array in host memory or an int device pointer) -- the state ``frames`` FRAME passes of
        ``refine`` leave, traced over the 8x8 tiles that hold a selected pixel only.  Blocking."""
        if isinstance(mask, np.ndarray):
            mask = np.ascontiguousarray(mask, dtype=np.uint32)
            assert mask.size >= self.mask_words
            ptr = mask.ctypes.data
        else:
            ptr = int(mask)
        st = _lib.RefineTilesStats()
        self._check(self.lib.hrt_refine_tiles(self.handle, ctypes.byref(pc), ctypes.c_void_p(ptr), int(max_history),
                                              int(frames), _lib.REFINE_MOMENTS if moments else 0,
                                              ctypes.byref(st) if want_stats else None), "hrt_refine_tiles")
        return st if want_stats else None

    def refine_tiles_until(self, pc: _lib.PushConstants, max_history: int, max_passes: int, frames_per_pass: int = 1,
                           guide_ptr: Optional[int] = None, rule: Optional[_lib.RefineRule] = None, **fields):
        """hrt_refine_tiles_until: select, then one tile-masked pass of ``frames_per_pass`` frames, until nothing is
        selected or max_passes have run; pass k starts at rng_offset pc.rng_offset + k * frames_per_pass.  Returns
        (passes done, pixel-frames folded, settled)."""
        rule = rule if rule is not None else self.refine_rule(**fields)
        passes, frames, settled = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self.lib.hrt_refine_tiles_until(self.handle, ctypes.byref(pc), ctypes.byref(rule),
                                                    ctypes.c_void_p(guide_ptr or 0), int(max_history), int(max_passes),
                                                    int(frames_per_pass), _lib.REFINE_MOMENTS, ctypes.byref(passes),
                                                    ctypes.byref(frames), ctypes.byref(settled)), "hrt_refine_tiles_until")
        return passes.value, frames.value, bool(settled.value)

    # ---- the variance-guided denoise (hrt_denoise_variance and the moments calls) ----

    def variance_info(self, iterations: Optional[int] = None, method: int = _lib.VARIANCE_AUTO,
                      min_history: Optional[int] = None, sigma_variance: Optional[float] = None,
                      variance_floor: Optional[float] = None, sigma_normal: Optional[float] = None,
                      sigma_depth: Optional[float] = None) -> _lib.VarianceInfo:
        """hrt_variance_defaults with the given fields replaced (None: the default)."""
        info = _lib.VarianceInfo()
        self.lib.hrt_variance_defaults(ctypes.byref(info))
        info.method = int(method)
        if iterations is not None:
            info.iterations = int(iterations)
        if min_history is not None:
            info.min_history = int(min_history)
        for name, v in (("sigma_variance", sigma_variance), ("variance_floor", variance_floor),
                        ("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth)):
            if v is not None:
                setattr(info, name, float(v))
        return info

    def accumulate_history_moments(self, max_history: int) -> None:
        """hrt_accumulate_history_moments: ``accumulate_history``, and the trace image's luminance moments folded
        into the moments image with the same per-pixel counts."""
        self._check(self.lib.hrt_accumulate_history_moments(self.handle, int(max_history)),
                    "hrt_accumulate_history_moments")

    def reproject_moments(self, prev: "View", prev_hits_ptr: int, cur: "View", cur_hits_ptr: int,
                          info: Optional[_lib.ReprojectInfo] = None, **fields) -> None:
        """hrt_reproject_moments: ``reproject``, and the moments image carried through the same taps (cleared where
        a pixel is rejected).  Mixing the plain and the moments calls leaves stale moments."""
        info = info if info is not None else self.reproject_info(**fields)
        self._check(self.lib.hrt_reproject_moments(self.handle, ctypes.byref(info), ctypes.byref(prev.record),
                                                   ctypes.c_void_p(prev_hits_ptr), ctypes.byref(cur.record),
                                                   ctypes.c_void_p(cur_hits_ptr)), "hrt_reproject_moments")

    # ---- object motion in the temporal history (hrt_reproject_motion[_moments]) ----

    @staticmethod
    def motion_tables(spheres=None, meshes=None):
        """(hrt_motion_tables, the arrays it points to) of two sequences of ``_lib.Motion`` records (None or empty:
        a NULL table with count 0).  Keep the second value alive until the call that takes the first has returned."""
        def arr(seq):
            seq = list(seq) if seq is not None else []
            return (_lib.Motion * len(seq))(*seq) if seq else None
        sa, ma = arr(spheres), arr(meshes)
        t = _lib.MotionTables(ctypes.addressof(sa) if sa is not None else None, len(sa) if sa is not None else 0,
                              ctypes.addressof(ma) if ma is not None else None, len(ma) if ma is not None else 0)
        return t, (sa, ma)

    def reproject_motion(self, prev: "View", prev_hits_ptr: int, cur: "View", cur_hits_ptr: int, spheres=None, meshes=None,
                         moments: bool = False, info: Optional[_lib.ReprojectInfo] = None, tables=None, **fields) -> None:
        """hrt_reproject_motion (moments: hrt_reproject_motion_moments): ``reproject`` / ``reproject_moments`` with a
        rigid motion per object -- ``spheres[i]`` for a hit of sphere i, ``meshes[m]`` for a hit of
        mesh m, ``_lib.Motion`` records as ``motion_between`` makes them; a missing entry is static.  ``tables``: an
        ``_lib.MotionTables`` instead.  The tables are copied before the call returns."""
        info = info if info is not None else self.reproject_info(**fields)
        keep = None
        if tables is None:
            tables, keep = self.motion_tables(spheres, meshes)
        name = "hrt_reproject_motion_moments" if moments else "hrt_reproject_motion"
        self._check(getattr(self.lib, name)(self.handle, ctypes.byref(info), ctypes.byref(tables), ctypes.byref(prev.record),
                                            ctypes.c_void_p(prev_hits_ptr), ctypes.byref(cur.record),
                                            ctypes.c_void_p(cur_hits_ptr)), name)
        del keep

    def fill_moments(self, m1: float, m2: float) -> None:
        """hrt_fill_moments: every pixel's moments = (m1, m2)."""
        self._check(self.lib.hrt_fill_moments(self.handle, float(m1), float(m2)), "hrt_fill_moments")

    def read_moments_into(self, dst_ptr: int, nbytes: int) -> None:
        """hrt_read_moments into caller memory (host or device pointer).  Blocking."""
        self._check(self.lib.hrt_read_moments(self.handle, ctypes.c_void_p(dst_ptr), int(nbytes)), "hrt_read_moments")

    def read_moments(self) -> np.ndarray:
        """hrt_read_moments: the moments image as float32 (local_rows, W, 2)."""
        out = np.empty((self.local_rows, self.width, 2), dtype=np.float32)
        self.read_moments_into(out.ctypes.data, out.nbytes)
        return out

    def denoise_variance_into(self, dst_ptr: int, nbytes: int, fmt: int = _lib.FMT_RGBA8, guide_ptr: Optional[int] = None,
                              variance_ptr: Optional[int] = None, variance_nbytes: int = 0,
                              info: Optional[_lib.VarianceInfo] = None, **fields) -> None:
        """hrt_denoise_variance into caller memory (host or device pointers): the variance-guided a-trous filter
         of the accumulator as local_rows x W texels of fmt and, with variance_ptr, the filtered
        variance as local_rows x W floats.  guide_ptr as ``denoise_into`` takes it; ``info`` or the fields of
        ``variance_info``.  Blocking."""
        info = info if info is not None else self.variance_info(**fields)
        self._check(self.lib.hrt_denoise_variance(self.handle, ctypes.byref(info), ctypes.c_void_p(guide_ptr or 0), int(fmt),
                                                  ctypes.c_void_p(dst_ptr), int(nbytes), ctypes.c_void_p(variance_ptr or 0),
                                                  int(variance_nbytes)), "hrt_denoise_variance")

    def denoise_variance(self, fmt: int = _lib.FMT_RGBA8, guide_ptr: Optional[int] = None, with_variance: bool = False,
                         info: Optional[_lib.VarianceInfo] = None, **fields):
        """hrt_denoise_variance: the filtered accumulator as uint8 or float32 (local_rows, W, 4); with_variance:
        (image, variance float32 (local_rows, W))."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.uint8 if fmt == _lib.FMT_RGBA8 else np.float32)
        var = np.empty((self.local_rows, self.width), dtype=np.float32) if with_variance else None
        self.denoise_variance_into(out.ctypes.data, out.nbytes, fmt, guide_ptr, var.ctypes.data if with_variance else None,
                                   var.nbytes if with_variance else 0, info, **fields)
        return (out, var) if with_variance else out

    def denoise_variance_present(self, dst_ptr: int, nbytes: int, width: int, height: int, pitch: Optional[int] = None,
                                 fmt: int = _lib.PRESENT_B8G8R8A8, guide_ptr: Optional[int] = None,
                                 info: Optional[_lib.VarianceInfo] = None, **fields) -> int:
        """hrt_denoise_variance_present: the filter, then ``present`` of the filtered accumulator (same target
        rules, same ticket sequence); returns the ticket without waiting."""
        info = info if info is not None else self.variance_info(**fields)
        target, t = self._present_info(_lib.IMG_ACCUM, width, height, pitch, fmt), ctypes.c_uint64()
        self._check(self.lib.hrt_denoise_variance_present(self.handle, ctypes.byref(info), ctypes.c_void_p(guide_ptr or 0),
                                                          ctypes.byref(target), ctypes.c_void_p(dst_ptr), int(nbytes),
                                                          ctypes.byref(t)), "hrt_denoise_variance_present")
        return t.value

    # ---- ray queries (hrt_intersect, hrt_intersect_primary) ----

    @staticmethod
    def ray_queries(origins, directions, t_max=None) -> np.ndarray:
        """n hrt_ray_query records (_lib.RAY_QUERY_DTYPE) of origins[n, 3], directions[n, 3] (any length:
        the library normalises them) and t_max (None: FLT_MAX; a scalar or n values)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("origins and directions differ in length")
        rays = np.zeros(len(o), dtype=_lib.RAY_QUERY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        rays["t_max"] = np.finfo(np.float32).max if t_max is None else np.asarray(t_max, np.float32)
        return rays

    def intersect_into(self, rays_ptr: int, n: int, hits_ptr: int, method: int = _lib.QUERY_AUTO,
                       with_stats: bool = False):
        """hrt_intersect on caller memory: n hrt_ray_query records at rays_ptr -> n hrt_hit records at
        hits_ptr (host pointers, or 16-byte aligned pointers into the context's device, e.g. a torch tensor's
        data_ptr()).  Blocking.  Returns the call's _lib.QueryStats when with_stats, else None."""
        st = _lib.QueryStats()
        self._check(self.lib.hrt_intersect(self.handle, ctypes.c_void_p(rays_ptr), int(n), int(method),
                                           ctypes.c_void_p(hits_ptr), ctypes.byref(st) if with_stats else None),
                    "hrt_intersect")
        return st if with_stats else None

    def intersect(self, origins, directions, t_max=None, method: int = _lib.QUERY_AUTO, with_stats: bool = False):
        """hrt_intersect: the closest hit of each ray (the reference's world_hit) as a
        structured array (_lib.HIT_DTYPE: t, kind 0 miss / 1 sphere / 2 triangle, index, mesh, normal).
        ``origins`` may also be a ready _lib.RAY_QUERY_DTYPE array (then ``directions`` is None).
        with_stats=True returns (hits, _lib.QueryStats)."""
        if directions is None:
            rays = np.ascontiguousarray(origins, dtype=_lib.RAY_QUERY_DTYPE)
        else:
            rays = self.ray_queries(origins, directions, t_max)
        hits = np.zeros(len(rays), dtype=_lib.HIT_DTYPE)
        st = self.intersect_into(rays.ctypes.data if len(rays) else 0, len(rays), hits.ctypes.data if len(rays) else 0,
                                 method, with_stats)
        return (hits, st) if with_stats else hits

    def intersect_primary(self, pc: _lib.PushConstants, rect=None, method: int = _lib.QUERY_AUTO,
                          with_stats: bool = False):
        """hrt_intersect_primary: the closest hit of the un-jittered primary ray of every pixel of rect =
        (x0, y0, w, h) (None: the whole image), as an (h, w) structured array (_lib.HIT_DTYPE).  Rows are
        trace-image rows (the present pass shows them flipped)."""
        x0, y0, w, h = (0, 0, self.width, self.height) if rect is None else (int(v) for v in rect)
        hits = np.zeros(max(w, 0) * max(h, 0), dtype=_lib.HIT_DTYPE)
        st = _lib.QueryStats()
        self._check(self.lib.hrt_intersect_primary(self.handle, ctypes.byref(pc), x0, y0, w, h, int(method),
                                                   _lib.ptr(hits), ctypes.byref(st) if with_stats else None),
                    "hrt_intersect_primary")
        hits = hits.reshape(h, w)
        return (hits, st) if with_stats else hits

    def intersect_primary_into(self, pc: _lib.PushConstants, hits_ptr: int, rect=None, method: int = _lib.QUERY_AUTO,
                               with_stats: bool = False):
        """hrt_intersect_primary into caller memory: w x h hrt_hit records, row-major, at hits_ptr (a host
        pointer, or a 16-byte aligned pointer into the context's device -- the guide of ``denoise`` when rect
        is None, without a round trip through the host).  Blocking.  Returns the call's _lib.QueryStats when
        with_stats, else None."""
        x0, y0, w, h = (0, 0, self.width, self.height) if rect is None else (int(v) for v in rect)
        st = _lib.QueryStats()
        self._check(self.lib.hrt_intersect_primary(self.handle, ctypes.byref(pc), x0, y0, w, h, int(method),
                                                   ctypes.c_void_p(hits_ptr), ctypes.byref(st) if with_stats else None),
                    "hrt_intersect_primary")
        return st if with_stats else None

    # ---- the first-hit pass (hrt_first_hits) ----

    def first_hits(self, pc: _lib.PushConstants, hits_device: int, method: int = _lib.FIRST_HITS_AUTO,
                   count: bool = False) -> None:
        """hrt_first_hits: the whole image's first hits -- ``intersect_primary_into``'s bytes -- into W x H
        hrt_hit records at hits_device, a 16-byte aligned pointer into the context's device.  Only enqueues, on
        the context's stream: ``reproject`` / ``denoise`` calls that follow read the result; keep the buffer
        until the pass has run.  count=True has the device count what ``first_hits_stats`` returns."""
        self._check(self.lib.hrt_first_hits(self.handle, ctypes.byref(pc), int(method),
                                            _lib.FIRST_HITS_COUNT if count else 0, ctypes.c_void_p(hits_device)),
                    "hrt_first_hits")

    def first_hits_stats(self) -> _lib.FirstHitsStats:
        """hrt_get_first_hits_stats: the record of the last ``first_hits(..., count=True)``.  Blocking."""
        st = _lib.FirstHitsStats()
        self._check(self.lib.hrt_get_first_hits_stats(self.handle, ctypes.byref(st)), "hrt_get_first_hits_stats")
        return st

    # ---- occlusion queries (hrt_occluded) ----

    def occluded_into(self, rays_ptr: int, n: int, bits_ptr: int, method: int = _lib.QUERY_AUTO,
                      with_stats: bool = False):
        """hrt_occluded on caller memory: n hrt_ray_query records at rays_ptr -> ceil(n / 32) uint32 words at
        bits_ptr, ray i as bit i & 31 of word i >> 5 (host pointers, or pointers into the context's device:
        rays 16-byte, bits 4-byte aligned, e.g. a torch tensor's data_ptr()).  Blocking.  Returns the call's
        _lib.OcclusionStats when with_stats, else None."""
        st = _lib.OcclusionStats()
        self._check(self.lib.hrt_occluded(self.handle, ctypes.c_void_p(rays_ptr), int(n), int(method),
                                          ctypes.c_void_p(bits_ptr), ctypes.byref(st) if with_stats else None),
                    "hrt_occluded")
        return st if with_stats else None

    def occluded(self, rays, method: int = _lib.QUERY_AUTO, with_stats: bool = False, packed: bool = False):
        """hrt_occluded: whether anything lies on each ray before its t_max -- True iff
        ``intersect`` of the same ray returns kind != 0 -- as a bool array of len(rays).  ``rays``: a
        _lib.RAY_QUERY_DTYPE array (``ray_queries``), or a torch tensor of n x 8 float32 on the host or on the
        context's device (anything with data_ptr() and shape).  packed=True returns the ceil(n / 32) uint32
        words instead (ray i: bit i & 31 of word i >> 5).  with_stats=True returns (result,
        _lib.OcclusionStats)."""
        if hasattr(rays, "data_ptr"):
            n, rays_ptr = int(rays.shape[0]), int(rays.data_ptr())
        else:
            rays = np.ascontiguousarray(rays, dtype=_lib.RAY_QUERY_DTYPE)
            n, rays_ptr = len(rays), rays.ctypes.data
        words = np.zeros((n + 31) // 32, np.uint32)
        st = self.occluded_into(rays_ptr if n else 0, n, words.ctypes.data if n else 0, method, with_stats)
        out = words if packed else np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
        return (out, st) if with_stats else out

    # ---- radiance queries (hrt_radiance) ----

    @staticmethod
    def radiance_queries(origins, seeds, centres) -> np.ndarray:
        """n hrt_radiance_query records (_lib.RADIANCE_QUERY_DTYPE) of origins[n, 3], seeds[n] (uint32) and
        centres[n, 3]."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
        if len(o) != len(c):
            raise ValueError("origins and centres differ in length")
        q = np.zeros(len(o), dtype=_lib.RADIANCE_QUERY_DTYPE)
        q["origin"], q["centre"] = o, c
        q["seed"] = np.asarray(seeds, np.uint32)
        return q

    def radiance_into(self, pc: _lib.PushConstants, queries_ptr: int, n: int, rgba_ptr: int,
                      method: int = _lib.QUERY_AUTO, with_stats: bool = False):
        """hrt_radiance on caller memory: n hrt_radiance_query records at queries_ptr -> n x 4 float32 at
        rgba_ptr (host pointers, or 16-byte aligned pointers into the context's device, e.g. a torch tensor's
        data_ptr()).  Blocking.  Returns the call's _lib.RadianceStats when with_stats, else None."""
        st = _lib.RadianceStats()
        self._check(self.lib.hrt_radiance(self.handle, ctypes.byref(pc), ctypes.c_void_p(queries_ptr), int(n),
                                          int(method), ctypes.c_void_p(rgba_ptr),
                                          ctypes.byref(st) if with_stats else None), "hrt_radiance")
        return st if with_stats else None

    def radiance(self, queries, pc: _lib.PushConstants, method: int = _lib.QUERY_AUTO, with_stats: bool = False):
        """hrt_radiance: what the path tracer returns for each query -- the reference's main()
        for a virtual pixel with trace_ray's root ``origin``, RNG state ``seed`` and sample centre ``centre``,
        under pc's matrix, jitter, sample and bounce counts -- as an (n, 4) float32 array, alpha 1.
        ``queries``: a _lib.RADIANCE_QUERY_DTYPE array (``radiance_queries``), or a torch tensor of n x 8
        32-bit words on the host or on the context's device (anything with data_ptr() and shape).
        with_stats=True returns (rgba, _lib.RadianceStats)."""
        if hasattr(queries, "data_ptr"):
            n, q_ptr = int(queries.shape[0]), int(queries.data_ptr())
        else:
            queries = np.ascontiguousarray(queries, dtype=_lib.RADIANCE_QUERY_DTYPE)
            n, q_ptr = len(queries), queries.ctypes.data
        rgba = np.zeros((n, 4), np.float32)
        st = self.radiance_into(pc, q_ptr if n else 0, n, rgba.ctypes.data if n else 0, method, with_stats)
        return (rgba, st) if with_stats else rgba

    def check_guards(self):
        """libhip_raytrace_debug.so: (guarded device buffers, buffers whose guard bands were overwritten)."""
        n, bad = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.hrt_debug_check_guards(self.handle, ctypes.byref(n), ctypes.byref(bad)),
                    "hrt_debug_check_guards")
        return n.value, bad.value

    def tile_lists(self, pc: _lib.PushConstants, refine: bool = True):
        """hrt_debug_tile_lists: the 8x8 tiles' primary triangle lists for a dispatch of pc, as
        (n[tiles], ok[tiles], entries[tiles, 64], tiles per row); entries are indices into the uploaded
        triangle buffer in list order (0xFFFFFFFF past n).  refine=False: the cap rule alone."""
        info = (ctypes.c_uint32 * 2)()
        self._check(self.lib.hrt_debug_tile_lists(self.handle, ctypes.byref(pc), 0, None, 0, info), "hrt_debug_tile_lists")
        out = np.zeros((info[0], _lib.TILE_LIST_WORDS), np.uint32)
        self._check(self.lib.hrt_debug_tile_lists(self.handle, ctypes.byref(pc), 1 if refine else 0, _lib.ptr(out),
                                                  out.size, info), "hrt_debug_tile_lists")
        return out[:, 0].copy(), out[:, 1] != 0, out[:, 2:].copy(), int(info[1])

    # ---- multi-GPU framebuffer gather (hrt_comm_*) ----

    @staticmethod
    def comm_unique_id() -> bytes:
        """A fresh RCCL unique id (rank 0 creates it and shares the bytes, e.g. by torch.distributed)."""
        lib = _lib.load()
        buf = (ctypes.c_uint8 * _lib.COMM_ID_BYTES)()
        _lib.check(lib.hrt_comm_unique_id(buf), "hrt_comm_unique_id", None, lib)
        return bytes(buf)

    def comm_init(self, uid: bytes, rank: int, world: int):
        """Join the RCCL communicator of a world-way partition (collective over the ranks)."""
        buf = (ctypes.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(uid)
        self._check(self.lib.hrt_comm_init(self.handle, buf, int(rank), int(world)), "hrt_comm_init")

    @staticmethod
    def comm_init_all(ctxs):
        """One process driving every part: ctxs[i] is part i of len(ctxs)."""
        lib = ctxs[0].lib
        arr = (ctypes.c_void_p * len(ctxs))(*[c.handle.value for c in ctxs])
        _lib.check(lib.hrt_comm_init_all(arr, len(ctxs)), "hrt_comm_init_all", None, lib)

    def comm_info(self):
        """(rank, world, transport) of the context's communicator."""
        r, w, t = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.hrt_comm_info(self.handle, ctypes.byref(r), ctypes.byref(w), ctypes.byref(t)),
                    "hrt_comm_info")
        return r.value, w.value, t.value

    def read_frame(self, image_id: int, fmt: int = _lib.FMT_RGBA8, root: bool = True):
        """The gathered full frame (height, W, 4) through hrt_read_image on a context with a
        communicator; ranks other than the root pass root=False and get None."""
        if not root:
            self._check(self.lib.hrt_read_image(self.handle, image_id, fmt, None, 0), "hrt_read_image")
            return None
        dt = np.uint8 if fmt == _lib.FMT_RGBA8 else np.float32
        out = np.empty((self.height, self.width, 4), dtype=dt)
        self._check(self.lib.hrt_read_image(self.handle, image_id, fmt, _lib.ptr(out), out.nbytes), "hrt_read_image")
        return out

    def global_rows(self) -> np.ndarray:
        """Global row index of each local row (rows >= height are padding)."""
        lr = np.arange(self.local_rows, dtype=np.int64)
        if self.part_count <= 1:
            return lr
        t = lr // self.row_tile
        return (t * self.part_count + self.part_index) * self.row_tile + lr % self.row_tile


class Image:
    """What RayTracePipeline::image / DiffusePipeline::image hand to the presenter."""

    def __init__(self, ctx: HrtContext, image_id: int):
        self.ctx, self.image_id = ctx, image_id

    def read(self, fmt: int = _lib.FMT_RGBA8) -> Optional[np.ndarray]:
        """What the presenter gets.  Without a communicator: the context's rows.  On a context joined to
        one (hrt_comm_init): the gathered FULL frame -- a collective every rank must call; ranks other
        than 0 get None.  On a group (hrt_comm_init_all): the full frame (a blocking read; the root's
        HrtContext.present / RenderPassOverFrame.render shows the same frame without a host wait)."""
        rank, _, transport = self.ctx.comm_info()
        if transport == _lib.COMM_NONE:
            return self.ctx.read(self.image_id, fmt)
        return self.ctx.read_frame(self.image_id, fmt, root=transport != _lib.COMM_RCCL or rank == 0)


@dataclass
class PresentTarget:
    """The memory a frame is presented into (the reference's swapchain image view): ``ptr`` is a device
    pointer a kernel may write (an import of the context, device, managed or registered host memory),
    ``nbytes`` the bytes that may be written from it."""
    ptr: int
    nbytes: int
    width: int
    height: int
    pitch: Optional[int] = None  # bytes per row; None = width * 4
    format: int = _lib.PRESENT_B8G8R8A8


class RenderPassOverFrame:
    """src/texture_draw_pipeline.rs:96-157 on the HIP context: the image drawn as a nearest-sampled,
    vertically flipped quad over the whole target (hrt_present).  With ctx the root of a comm_init_all
    group, the view is the group's full frame (the gathered present)."""

    def __init__(self, ctx: HrtContext, output_format: int = _lib.PRESENT_B8G8R8A8):
        self.ctx, self.output_format = ctx, int(output_format)

    def render(self, view: Image, target: PresentTarget) -> int:
        """Enqueues the pass after the work issued so far (the reference's before_future) and returns
        its ticket (the after_future): wait with ctx.present_wait, poll with ctx.present_done."""
        if view.ctx is not self.ctx:
            raise ValueError("view must be an image of the render pass's context")
        if target.format != self.output_format:
            raise ValueError("the target's format differs from the render pass's output format")
        return self.ctx.present(view.image_id, target.ptr, target.nbytes, target.width, target.height, target.pitch,
                                target.format)

    def render_denoised(self, view: Image, target: PresentTarget, guide_ptr: Optional[int] = None, **fields) -> int:
        """``render`` with the denoise pass between the image and the quad (hrt_denoise_present): guide_ptr as
        ``HrtContext.denoise_into`` takes it (``RayTracePipeline.first_hits_into``), ``fields`` those of
        ``HrtContext.denoise_info`` (iterations, method, sigmas).  Returns the ticket."""
        if view.ctx is not self.ctx:
            raise ValueError("view must be an image of the render pass's context")
        if target.format != self.output_format:
            raise ValueError("the target's format differs from the render pass's output format")
        return self.ctx.denoise_present(target.ptr, target.nbytes, target.width, target.height, target.pitch,
                                        target.format, guide_ptr, image_id=view.image_id, **fields)

    def render_variance_denoised(self, view: Image, target: PresentTarget, guide_ptr: Optional[int] = None, **fields) -> int:
        """``render`` with the variance-guided denoise between the accumulator and the quad
        (hrt_denoise_variance_present): view must be the accumulated image, ``fields`` those of
        ``HrtContext.variance_info``.  Returns the ticket."""
        if view.ctx is not self.ctx or view.image_id != _lib.IMG_ACCUM:
            raise ValueError("view must be the accumulated image of the render pass's context")
        if target.format != self.output_format:
            raise ValueError("the target's format differs from the render pass's output format")
        return self.ctx.denoise_variance_present(target.ptr, target.nbytes, target.width, target.height, target.pitch,
                                                 target.format, guide_ptr, **fields)


    def render_upsampled(self, view: Image, target: PresentTarget, low_hits_ptr: int, high_hits_ptr: int,
                         producer: Optional[HrtContext] = None, **fields) -> int:
        """``render`` of a view traced below the target's size (hrt_upsample_present): the image reconstructed at
        target.width x target.height, guided by the view's own first hits (low_hits_ptr) and the target-size ones
        (high_hits_ptr) of the same camera.  ``producer``: the context whose stream wrote high_hits_ptr -- the pass
        is ordered after it (``HrtContext.order_after``).  ``fields`` as ``HrtContext.upsample_present`` takes them
        (footprint, sigmas, denoise, variance).  Returns the ticket."""
        if view.ctx is not self.ctx:
            raise ValueError("view must be an image of the render pass's context")
        if target.format != self.output_format:
            raise ValueError("the target's format differs from the render pass's output format")
        if producer is not None:
            self.ctx.order_after(producer)
        return self.ctx.upsample_present(target.ptr, target.nbytes, target.width, target.height, low_hits_ptr,
                                         high_hits_ptr, target.pitch, target.format, image_id=view.image_id, **fields)


# ---- pipelines ---------------------------------------------------------------------------------

class RayTracePipeline:
    """src/raytrace_pipeline.rs:31-266 on the HIP context."""

    def __init__(self, ctx: HrtContext, image_size, settings: RayTracerSettings):
        self.ctx = ctx
        self.image_size = (int(image_size[0]), int(image_size[1]))
        rays, num_rays, jitter = create_rays(self.image_size, settings.camera_focal_length, settings.viewport_height,
                                             settings.up)
        spheres = sphere_records(settings.sphere_data)
        tris, meshes = transform_meshes(settings.mesh_data if settings.mesh_data else [get_null_mesh()])
        n_meshes = len(settings.mesh_data)
        self.ray_count = num_rays
        self.sphere_count = len(settings.sphere_data)
        self.mesh_count = n_meshes
        self.num_samples = max(int(settings.num_samples), 1)       # :88
        self.max_bounces = max(int(settings.max_bounces), 0)       # :89
        self.use_environment_lighting = bool(settings.use_environment_lighting)
        self.sample_jitter = float(np.float32(settings.sample_jitter if settings.sample_jitter is not None else jitter))
        self.rays, self.tris, self.meshes, self.spheres = rays[:num_rays], tris, meshes[:n_meshes], spheres
        ctx.set_scene(rays[:num_rays], spheres, tris, meshes[:n_meshes])
        self.grid = ray_grid(self.image_size, settings.camera_focal_length, settings.viewport_height, settings.up)[:3]

    def image(self) -> Image:
        return Image(self.ctx, _lib.IMG_TRACE)

    def shift_rays(self, ox: float, oy: float) -> None:
        """The pipeline's ray grid shifted by (ox, oy) pixels for the frames that follow (hrt_set_ray_grid; stream
        ordered, no host wait): (0, 0) restores the rays the pipeline was made with, bit for bit."""
        self.ctx.shift_ray_grid(ox, oy, self.grid)

    def push_constants(self, camera: Camera, rng_offset: int, init: bool) -> _lib.PushConstants:
        """The 124-byte block of dispatch(), src/raytrace_pipeline.rs:243-257."""
        pc = _lib.PushConstants()
        pos = np.asarray(camera.position, np.float32)
        pc.cam_pos[:] = [float(pos[0]), float(pos[1]), float(pos[2]), 1.0]
        pc.cam_alignment_mat[:] = [float(v) for v in view_matrix(camera.direction, camera.up)]
        pc.num_rays = self.ray_count
        pc.num_spheres = self.sphere_count
        pc.num_meshes = self.mesh_count
        pc.num_samples = self.num_samples
        pc.jitter_size = self.sample_jitter
        pc.max_bounces = self.max_bounces
        pc.use_environment_light = int(self.use_environment_lighting)
        pc.rng_offset = int(rng_offset) & 0xFFFFFFFF
        pc.init = int(bool(init))
        pc.width, pc.height = self.image_size
        return pc

    def compute(self, camera: Camera, rng_offset: int) -> None:
        self.ctx.trace(self.push_constants(camera, rng_offset, False))

    def first_hits(self, camera: Camera, rect=None) -> np.ndarray:
        """The first-hit buffer of a view: the closest hit (t, kind, index, mesh, normal; _lib.HIT_DTYPE) of
        the un-jittered primary ray of every pixel of rect = (x0, y0, w, h) (None: the whole image), as an
        (h, w) array in trace-image rows (hrt_intersect_primary)."""
        return self.ctx.intersect_primary(self.push_constants(camera, 0, False), rect)

    def first_hits_into(self, camera: Camera, ptr: int) -> None:
        """``first_hits`` of the whole image written to W x H hrt_hit records at ptr (host, or 16-byte aligned
        device memory of the context): the guide of ``DiffusePipeline.denoised`` /
        ``RenderPassOverFrame.render_denoised``, kept on the device."""
        self.ctx.intersect_primary_into(self.push_constants(camera, 0, False), ptr)

    def first_hits_async(self, camera: Camera, hits_device: int, method: int = _lib.FIRST_HITS_AUTO,
                         count: bool = False) -> None:
        """``first_hits_into`` for device memory without the host wait (hrt_first_hits): enqueued on the
        context's stream, so the ``reproject`` / ``denoised`` calls that follow read it; keep the buffer until
        the pass has run.  count=True: ``self.ctx.first_hits_stats()`` afterwards."""
        self.ctx.first_hits(self.push_constants(camera, 0, False), hits_device, method, count)

    def pick(self, camera: Camera, x: int, y: int):
        """What lies under pixel (x, y) of the view: one hit record (numpy.void of _lib.HIT_DTYPE).  x, y are
        trace-image coordinates; the present pass flips rows, so a pixel of a presented height-H target is
        row H - 1 - y here."""
        return self.first_hits(camera, (int(x), int(y), 1, 1))[0, 0]

    @staticmethod
    def segment_rays(a, b) -> np.ndarray:
        """The rays of the segments a[i] -> b[i] (_lib.RAY_QUERY_DTYPE): origin a, direction b - a, t_max =
        |b - a|, every step in binary32 (the squares summed x, y, z in order, then the square root)."""
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 3)
        d = b - a
        sq = d * d
        length = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2], dtype=np.float32)
        return HrtContext.ray_queries(a, d, length)

    def visible(self, a, b, method: int = _lib.QUERY_AUTO) -> np.ndarray:
        """Whether b[i] is visible from a[i]: nothing of the scene on the open segment between them that the
        reference's world_hit accepts (0.001 < dist < |b - a|).  ~occluded(segment_rays(a, b))."""
        return ~self.ctx.occluded(self.segment_rays(a, b), method)

    def pixel_queries(self, camera: Camera, xs, ys, frame: int) -> np.ndarray:
        """The radiance queries (_lib.RADIANCE_QUERY_DTYPE) of pixels (xs[i], ys[i]) of the frame that
        ``compute(camera, frame)`` traces: origin the camera position, seed frame * 719393 + id, centre the
        ray centre of id = x + y * width."""
        w, h = self.image_size
        xs = np.asarray(xs, np.int64).reshape(-1)
        ys = np.asarray(ys, np.int64).reshape(-1)
        if len(xs) != len(ys) or (len(xs) and (xs.min() < 0 or xs.max() >= w or ys.min() < 0 or ys.max() >= h)):
            raise ValueError("pixel coordinates outside the image")
        ids = xs + ys * w
        seeds = ((int(frame) & 0xFFFFFFFF) * 719393 + ids) & 0xFFFFFFFF
        origins = np.broadcast_to(np.asarray(camera.position, np.float32)[:3], (len(ids), 3))
        return HrtContext.radiance_queries(origins, seeds, self.rays["sample_centre"][ids, :3])

    def radiance_pixels(self, camera: Camera, xs, ys, frame: int, method: int = _lib.QUERY_AUTO) -> np.ndarray:
        """What ``compute(camera, frame)`` stores at pixels (xs[i], ys[i]) of an RGBA32F trace image, bit for
        bit, as an (n, 4) float32 array -- without tracing the frame (hrt_radiance on ``pixel_queries``)."""
        return self.ctx.radiance(self.pixel_queries(camera, xs, ys, frame), self.push_constants(camera, frame, False),
                                 method)

    def init(self) -> None:
        self.ctx.trace(self.push_constants(Camera(), 0, True))


class DiffusePipeline:
    """src/diffuse.rs:22-136: the progressive accumulator (image_combiner.glsl)."""

    def __init__(self, ctx: HrtContext, image_size):
        self.ctx = ctx
        self.image_size = (int(image_size[0]), int(image_size[1]))

    def image(self) -> Image:
        return Image(self.ctx, _lib.IMG_ACCUM)

    def next_frame(self, frame_num: int, next_image: Image) -> None:
        if next_image.ctx is not self.ctx or next_image.image_id != _lib.IMG_TRACE:
            raise ValueError("next_image must be the trace image of the same context")
        self.ctx.accumulate(frame_num)

    def next_frame_history(self, next_image: Image, max_history: int = 32, moments: bool = False) -> None:
        """``next_frame`` with per-pixel frame counts (hrt_accumulate_history; not a reference feature): after a
        camera move, ``HrtContext.reproject`` first, then this -- a pixel whose surface point the old view
        held keeps its history, the others start again with this frame.  moments: also fold the frame's
        luminance moments (hrt_accumulate_history_moments, with ``HrtContext.reproject_moments`` after a move),
        what ``variance_denoised`` filters by."""
        if next_image.ctx is not self.ctx or next_image.image_id != _lib.IMG_TRACE:
            raise ValueError("next_image must be the trace image of the same context")
        if moments:
            self.ctx.accumulate_history_moments(max_history)
        else:
            self.ctx.accumulate_history(max_history)

    def reproject_history(self, prev: "View", prev_hits_ptr: int, cur: "View", cur_hits_ptr: int, motion=None,
                          moments: bool = False, **fields) -> None:
        """The reprojection that precedes ``next_frame_history`` after a move: ``HrtContext.reproject[_moments]``, or,
        with motion = (spheres, meshes) -- two sequences of ``motion_between`` records, either may be None -- the
        form that follows moving objects (``HrtContext.reproject_motion``)."""
        if motion is not None:
            self.ctx.reproject_motion(prev, prev_hits_ptr, cur, cur_hits_ptr, motion[0], motion[1], moments, **fields)
        elif moments:
            self.ctx.reproject_moments(prev, prev_hits_ptr, cur, cur_hits_ptr, **fields)
        else:
            self.ctx.reproject(prev, prev_hits_ptr, cur, cur_hits_ptr, **fields)

    def next_frame_history_from(self, next_image: Image, offset=(0.0, 0.0), max_history: Optional[int] = None,
                                moments: bool = False, fill: Optional[bool] = None, source_hits_ptr: Optional[int] = None,
                                hits_ptr: Optional[int] = None) -> None:
        """``next_frame_history`` with the trace image of another context, usually a smaller one whose ray grid was
        shifted by ``offset`` (``HrtContext.shift_ray_grid`` with ``history_phase``) before the trace
        (hrt_accumulate_history_from): over nx * ny frames every pixel of this image takes a sample of its own."""
        if next_image.image_id != _lib.IMG_TRACE:
            raise ValueError("next_image must be a trace image")
        self.ctx.accumulate_history_from(next_image.ctx, offset, max_history, moments, fill, source_hits_ptr, hits_ptr)

    def refine_until(self, pipeline: "RayTracePipeline", camera: "Camera", first_frame: int, max_passes: int,
                     max_history: int = 1 << 24, guide_ptr: Optional[int] = None, method: int = _lib.REFINE_AUTO,
                     **rule):
        """Adaptive refinement of the accumulated image (hrt_refine_until; not a reference feature): passes of new
        samples for the pixels whose estimate is still noisy, with the frames ``first_frame``, + 1, ... of
        ``pipeline`` under ``camera`` -- frames beyond those the history already holds (``next_frame_history`` with
        moments=True).  ``rule``: the fields of ``HrtContext.refine_rule``.  Returns (passes done, pixel-frames
        traced, settled)."""
        if pipeline.ctx is not self.ctx:
            raise ValueError("pipeline must trace on the same context")
        return self.ctx.refine_until(pipeline.push_constants(camera, first_frame, False), max_history, max_passes,
                                     guide_ptr, method, **rule)

    def refine_tiles_until(self, pipeline: "RayTracePipeline", camera: "Camera", first_frame: int, max_passes: int,
                           frames_per_pass: int = 1, max_history: int = 1 << 24, guide_ptr: Optional[int] = None, **rule):
        """``refine_until`` through the tile-masked passes (hrt_refine_tiles_until): each pass traces only the 8x8
        tiles that hold a selected pixel, ``frames_per_pass`` frames at once; pass k uses the frames ``first_frame +
        k * frames_per_pass`` onwards.  Returns (passes done, pixel-frames folded, settled)."""
        if pipeline.ctx is not self.ctx:
            raise ValueError("pipeline must trace on the same context")
        return self.ctx.refine_tiles_until(pipeline.push_constants(camera, first_frame, False), max_history, max_passes,
                                           frames_per_pass, guide_ptr, **rule)

    def variance_denoised(self, guide_ptr: Optional[int] = None, fmt: int = _lib.FMT_RGBA8, **fields) -> np.ndarray:
        """The accumulated image through the variance-guided denoise (hrt_denoise_variance), as uint8 or float32
        (H, W, 4); ``fields`` as ``HrtContext.variance_info`` takes them."""
        return self.ctx.denoise_variance(fmt, guide_ptr, **fields)

    def denoised(self, guide_ptr: Optional[int] = None, fmt: int = _lib.FMT_RGBA8, **sigmas) -> np.ndarray:
        """The accumulated image through the denoise pass (hrt_denoise), as uint8 or float32 (H, W, 4):
        guide_ptr = the view's first hits on the device (``RayTracePipeline.first_hits_into``) or None for the
        colour-only filter; ``sigmas`` (and iterations / method) as ``HrtContext.denoise_info`` takes them."""
        return self.ctx.denoise(fmt, guide_ptr, image_id=_lib.IMG_ACCUM, **sigmas)
