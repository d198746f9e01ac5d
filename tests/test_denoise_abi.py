"""The denoise pass on the CPU: the layout of hrt_denoise_info (a compiled C probe against the ctypes mirror),
the exports of both libraries, hrt_denoise_defaults, the Python constants and the NULL-handle rejection."""
import ctypes
import os
import subprocess

import numpy as np

import denoise_ref as D
from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("image_id", "iterations", "method", "flags", "sigma_colour", "sigma_normal", "sigma_depth", "reserved")
NAMES = {"hrt_denoise_defaults", "hrt_denoise", "hrt_denoise_present"}


def test_struct_layout_and_constants(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %d %d %d %u\\n", sizeof(hrt_denoise_info), (int)HRT_DENOISE_AUTO,\n'
                   '         (int)HRT_DENOISE_DIRECT, (int)HRT_DENOISE_TILED, HRT_ABI_VERSION);\n'
                   '  printf("%.9g %.9g %.9g\\n", (double)HRT_DENOISE_SIGMA_COLOUR, (double)HRT_DENOISE_SIGMA_NORMAL,\n'
                   '         (double)HRT_DENOISE_SIGMA_DEPTH);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_denoise_info, {f}));\n' for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:5]] == [32, 0, 1, 2, 6]  # additive: the ABI version stays 6
    assert tuple(float(v) for v in out[5:8]) == _lib.DENOISE_SIGMAS == D.DEFAULT_SIGMAS
    want = [0, 4, 8, 12, 16, 20, 24, 28]
    assert [int(v) for v in out[8:]] == want
    assert [n for n, _ in _lib.DenoiseInfo._fields_] == list(FIELDS)
    assert [getattr(_lib.DenoiseInfo, f).offset for f in FIELDS] == want and ctypes.sizeof(_lib.DenoiseInfo) == 32
    assert (_lib.DENOISE_AUTO, _lib.DENOISE_DIRECT, _lib.DENOISE_TILED, _lib.ABI_VERSION) == (0, 1, 2, 6)
    assert _lib.DENOISE_MAX_ITERATIONS == 5 and set(_lib.DENOISE_NAMES) == {0, 1, 2}


def test_symbols_exported_from_both_libraries():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
        assert NAMES <= exported, path
    assert NAMES <= set(_lib.EXPORTED_SYMBOLS)
    for lib in (_lib.load(), _lib.load(debug=True)):
        assert lib.hrt_denoise.argtypes and lib.hrt_denoise_present.argtypes and lib.hrt_denoise_defaults.argtypes


def test_kernels_are_in_the_code_object():
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"denoise_prep", b"atrous_direct", b"atrous_tiled"):
        assert k in blob, k


def test_defaults():
    for lib in (_lib.load(), _lib.load(debug=True)):
        info = _lib.DenoiseInfo(9, 9, 9, 9, -1.0, -1.0, -1.0, 9)
        lib.hrt_denoise_defaults(ctypes.byref(info))
        assert (info.image_id, info.iterations, info.method, info.flags, info.reserved) == (_lib.IMG_ACCUM, 5,
                                                                                            _lib.DENOISE_AUTO, 0, 0)
        assert (info.sigma_colour, info.sigma_normal, info.sigma_depth) == _lib.DENOISE_SIGMAS
        lib.hrt_denoise_defaults(None)  # ignored


def test_null_handles_are_rejected():
    lib = _lib.load()
    info = _lib.DenoiseInfo()
    lib.hrt_denoise_defaults(ctypes.byref(info))
    dst = np.full(64, 7, np.uint8)
    assert lib.hrt_denoise(None, ctypes.byref(info), None, _lib.FMT_RGBA8, _lib.ptr(dst), dst.nbytes) == 1
    target, ticket = _lib.PresentInfo(_lib.IMG_ACCUM, 0, 4, 4, 16, 0), ctypes.c_uint64(77)
    assert lib.hrt_denoise_present(None, ctypes.byref(info), None, ctypes.byref(target), _lib.ptr(dst), dst.nbytes,
                                   ctypes.byref(ticket)) == 1
    assert (dst == 7).all() and ticket.value == 77  # nothing written
