"""Temporal history on the CPU: the layouts of hrt_view and hrt_reproject_info (a compiled C probe against the
ctypes mirrors), the exports of both libraries, hrt_reproject_defaults, the Python constants, the View helper
and the NULL-handle rejection."""
import ctypes
import os
import subprocess

import numpy as np

import history_ref as H
import epq_raytracer_amd as E
from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_FIELDS = ("cam_pos", "cam_alignment_mat", "grid_first", "grid_dx", "grid_dy")
INFO_FIELDS = ("filter", "flags", "depth_tolerance", "min_normal_dot", "reserved")
NAMES = {"hrt_reproject_defaults", "hrt_reproject", "hrt_accumulate_history", "hrt_fill_history", "hrt_read_history"}


def test_struct_layouts_and_constants(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %zu %d %d %u %u\\n", sizeof(hrt_view), sizeof(hrt_reproject_info),\n'
                   '         (int)HRT_REPROJECT_NEAREST, (int)HRT_REPROJECT_BILINEAR, HRT_HISTORY_MAX, HRT_ABI_VERSION);\n'
                   '  printf("%.9g %.9g\\n", (double)HRT_REPROJECT_DEPTH_TOLERANCE, (double)HRT_REPROJECT_MIN_NORMAL_DOT);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_view, {f}));\n' for f in VIEW_FIELDS)
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_reproject_info, {f}));\n' for f in INFO_FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:6]] == [128, 32, 0, 1, 1 << 24, 6]  # additive: the ABI version stays 6
    defaults = tuple(float(np.float32(v)) for v in out[6:8])
    assert defaults == tuple(float(np.float32(v)) for v in _lib.REPROJECT_DEFAULTS)
    assert _lib.REPROJECT_DEFAULTS == H.DEFAULTS
    want_view, want_info = [0, 16, 80, 96, 112], [0, 4, 8, 12, 16]
    assert [int(v) for v in out[8:13]] == want_view and [int(v) for v in out[13:]] == want_info
    assert [n for n, _ in _lib.View._fields_] == list(VIEW_FIELDS)
    assert [n for n, _ in _lib.ReprojectInfo._fields_] == list(INFO_FIELDS)
    assert [getattr(_lib.View, f).offset for f in VIEW_FIELDS] == want_view and ctypes.sizeof(_lib.View) == 128
    assert [getattr(_lib.ReprojectInfo, f).offset for f in INFO_FIELDS] == want_info
    assert ctypes.sizeof(_lib.ReprojectInfo) == 32
    assert (_lib.REPROJECT_NEAREST, _lib.REPROJECT_BILINEAR, _lib.HISTORY_MAX, _lib.ABI_VERSION) == (0, 1, 1 << 24, 6)
    assert (H.NEAREST, H.BILINEAR) == (0, 1) and set(_lib.REPROJECT_NAMES) == {0, 1}


def test_symbols_exported_from_both_libraries():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
        assert NAMES <= exported, path
    assert NAMES <= set(_lib.EXPORTED_SYMBOLS)
    for lib in (_lib.load(), _lib.load(debug=True)):
        for n in NAMES:
            assert getattr(lib, n).argtypes, n


def test_kernels_are_in_the_code_object():
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"fold_history", b"reproject"):
        assert k in blob, k


def test_defaults():
    for lib in (_lib.load(), _lib.load(debug=True)):
        info = _lib.ReprojectInfo(9, 9, -1.0, -1.0, (ctypes.c_uint32 * 4)(9, 9, 9, 9))
        lib.hrt_reproject_defaults(ctypes.byref(info))
        assert (info.filter, info.flags, list(info.reserved)) == (_lib.REPROJECT_BILINEAR, 0, [0, 0, 0, 0])
        want = tuple(float(np.float32(v)) for v in _lib.REPROJECT_DEFAULTS)
        assert (info.depth_tolerance, info.min_normal_dot) == want
        lib.hrt_reproject_defaults(None)  # ignored


def test_view_helper_holds_the_push_block_camera_and_the_ray_grid():
    cam, settings = E.preset("box")
    size = (37, 23)
    v = E.View(cam, size, settings).record
    assert list(v.cam_pos) == [float(np.float32(c)) for c in cam.position] + [1.0]
    assert np.array_equal(np.array(v.cam_alignment_mat, np.float32), E.view_matrix(cam.direction, cam.up))
    rays, n, _ = E.create_rays(size, settings.camera_focal_length, settings.viewport_height, settings.up)
    first, dx, dy = (np.array(list(a)[:3], np.float32) for a in (v.grid_first, v.grid_dx, v.grid_dy))
    ys, xs = np.mgrid[0:size[1], 0:size[0]]
    centre = (first + dx * xs[..., None].astype(np.float32)) + dy * ys[..., None].astype(np.float32)
    assert n == size[0] * size[1]
    assert centre.reshape(-1, 3).tobytes() == np.ascontiguousarray(rays["sample_centre"][:n, :3]).tobytes()
    assert v.grid_first[3] == v.grid_dx[3] == v.grid_dy[3] == 0.0


def test_null_handles_are_rejected():
    lib = _lib.load()
    info, view = _lib.ReprojectInfo(), _lib.View()
    lib.hrt_reproject_defaults(ctypes.byref(info))
    dst = np.full(16, 7, np.uint32)
    assert lib.hrt_reproject(None, ctypes.byref(info), ctypes.byref(view), _lib.ptr(dst), ctypes.byref(view),
                             _lib.ptr(dst)) == 1
    assert lib.hrt_accumulate_history(None, 8) == 1 and lib.hrt_fill_history(None, 1) == 1
    assert lib.hrt_read_history(None, _lib.ptr(dst), dst.nbytes) == 1
    assert (dst == 7).all()  # nothing written
