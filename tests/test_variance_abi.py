"""The variance-guided denoise on the CPU: the layout of hrt_variance_info (a compiled C probe against the ctypes
mirror), the constants, the exports of both libraries, the kernels in the code object, hrt_variance_defaults and the
NULL-handle rejection."""
import ctypes
import os
import subprocess

import numpy as np

import variance_ref as V
from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("iterations", "method", "flags", "min_history", "sigma_variance", "variance_floor", "sigma_normal", "sigma_depth")
NAMES = {"hrt_variance_defaults", "hrt_accumulate_history_moments", "hrt_reproject_moments", "hrt_fill_moments",
         "hrt_read_moments", "hrt_denoise_variance", "hrt_denoise_variance_present"}


def test_struct_layout_and_constants(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %d %d %d %u %u\\n", sizeof(hrt_variance_info), (int)HRT_VARIANCE_AUTO,\n'
                   '         (int)HRT_VARIANCE_DIRECT, (int)HRT_VARIANCE_TILED, HRT_VARIANCE_MIN_HISTORY, HRT_ABI_VERSION);\n'
                   '  printf("%.9g %.9g\\n", (double)HRT_VARIANCE_SIGMA, (double)HRT_VARIANCE_FLOOR);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_variance_info, {f}));\n' for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:6]] == [32, 0, 1, 2, 4, 6]  # additive: the ABI version stays 6
    assert tuple(float(np.float32(v)) for v in out[6:8]) == (float(np.float32(4.0)), float(np.float32(1e-10)))
    want = [0, 4, 8, 12, 16, 20, 24, 28]
    assert [int(v) for v in out[8:]] == want
    assert [n for n, _ in _lib.VarianceInfo._fields_] == list(FIELDS)
    assert [getattr(_lib.VarianceInfo, f).offset for f in FIELDS] == want and ctypes.sizeof(_lib.VarianceInfo) == 32
    assert (_lib.VARIANCE_AUTO, _lib.VARIANCE_DIRECT, _lib.VARIANCE_TILED) == (0, 1, 2) and set(_lib.VARIANCE_NAMES) == {0, 1, 2}
    assert (_lib.VARIANCE_SIGMA, _lib.VARIANCE_FLOOR, _lib.VARIANCE_MIN_HISTORY, _lib.VARIANCE_MAX_ITERATIONS) == (4.0, 1e-10, 4, 5)
    assert V.DEFAULTS == (_lib.VARIANCE_SIGMA, _lib.VARIANCE_FLOOR, _lib.VARIANCE_MIN_HISTORY) + _lib.DENOISE_SIGMAS[1:]
    assert _lib.ABI_VERSION == 6


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
    for k in (b"fold_history_moments", b"fill_moments", b"variance_prep", b"atrous_variance_direct",
              b"atrous_variance_tiled", b"variance_store"):
        assert k in blob, k
    # reproject's moments instantiations beside the plain ones (Itanium mangling: ...Lj<filter>ELb<moments>E...)
    for filt in (0, 1):
        for moments in (0, 1):
            assert f"reprojectIjLj{filt}ELb{moments}E".encode() in blob, (filt, moments)


def test_defaults():
    for lib in (_lib.load(), _lib.load(debug=True)):
        info = _lib.VarianceInfo(9, 9, 9, 9, -1.0, -1.0, -1.0, -1.0)
        lib.hrt_variance_defaults(ctypes.byref(info))
        assert (info.iterations, info.method, info.flags, info.min_history) == (5, _lib.VARIANCE_AUTO, 0, 4)
        want = tuple(float(np.float32(v)) for v in (4.0, 1e-10) + _lib.DENOISE_SIGMAS[1:])
        assert (info.sigma_variance, info.variance_floor, info.sigma_normal, info.sigma_depth) == want
        lib.hrt_variance_defaults(None)  # ignored


def test_null_handles_are_rejected():
    lib = _lib.load()
    vinfo, rinfo, view, target = _lib.VarianceInfo(), _lib.ReprojectInfo(), _lib.View(), _lib.PresentInfo()
    lib.hrt_variance_defaults(ctypes.byref(vinfo))
    lib.hrt_reproject_defaults(ctypes.byref(rinfo))
    dst = np.full(16, 7, np.uint32)
    ticket = ctypes.c_uint64(5)
    assert lib.hrt_accumulate_history_moments(None, 8) == 1
    assert lib.hrt_reproject_moments(None, ctypes.byref(rinfo), ctypes.byref(view), _lib.ptr(dst), ctypes.byref(view),
                                     _lib.ptr(dst)) == 1
    assert lib.hrt_fill_moments(None, 0.0, 0.0) == 1
    assert lib.hrt_read_moments(None, _lib.ptr(dst), dst.nbytes) == 1
    assert lib.hrt_denoise_variance(None, ctypes.byref(vinfo), None, _lib.FMT_RGBA8, _lib.ptr(dst), dst.nbytes,
                                    _lib.ptr(dst), dst.nbytes) == 1
    assert lib.hrt_denoise_variance_present(None, ctypes.byref(vinfo), None, ctypes.byref(target), _lib.ptr(dst), dst.nbytes,
                                            ctypes.byref(ticket)) == 1
    assert (dst == 7).all() and ticket.value == 5  # nothing written
