"""Guided upsampling on the CPU: the layout of hrt_upsample_info (a compiled C probe against the ctypes mirror), the
constant, the defaults, the exports of both libraries, the kernels in the code object and the NULL-handle
rejection."""
import ctypes
import os
import subprocess

import numpy as np

from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("image_id", "width", "height", "footprint", "flags", "sigma_normal", "sigma_depth", "reserved")
NAMES = {"hrt_upsample_defaults", "hrt_upsample", "hrt_upsample_present", "hrt_order_after"}


def test_struct_layout_and_constant(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %u %u\\n", sizeof(hrt_upsample_info), HRT_UPSAMPLE_FOOTPRINT, HRT_ABI_VERSION);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_upsample_info, {f}));\n' for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [32, _lib.UPSAMPLE_FOOTPRINT, 6]  # additive: the ABI version stays 6
    assert _lib.UPSAMPLE_FOOTPRINT in (2, 4)
    offsets = [0, 4, 8, 12, 16, 20, 24, 28]
    assert out[3:] == offsets
    assert [n for n, _ in _lib.UpsampleInfo._fields_] == list(FIELDS)
    assert [getattr(_lib.UpsampleInfo, f).offset for f in FIELDS] == offsets
    assert ctypes.sizeof(_lib.UpsampleInfo) == 32 and _lib.ABI_VERSION == 6
    assert _lib.load().hrt_abi_version() == 6


def test_defaults():
    for lib in (_lib.load(), _lib.load(debug=True)):
        info = _lib.UpsampleInfo()
        ctypes.memset(ctypes.byref(info), 0xA5, 32)
        lib.hrt_upsample_defaults(ctypes.byref(info), 3840, 2160)
        assert (info.image_id, info.width, info.height, info.footprint, info.flags, info.reserved) == \
            (_lib.IMG_ACCUM, 3840, 2160, _lib.UPSAMPLE_FOOTPRINT, 0, 0)
        assert (info.sigma_normal, info.sigma_depth) == tuple(np.float32(_lib.DENOISE_SIGMAS[1:]))
        lib.hrt_upsample_defaults(None, 1, 1)  # a NULL info is ignored


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
    # Itanium mangling: upsample<Footprint, Out> with Out = float4 texels, RGBA8 words, the present target
    for footprint in (2, 4):
        for out in (0, 1, 2):
            k = b"_ZN3hrt8upsampleILi%dELi%dEEEv" % (footprint, out)
            assert k in blob, k
    # the passes it runs after are still there
    assert b"denoise_prep" in blob and b"atrous_direct" in blob and b"present_nearest" in blob


def test_null_handles_are_rejected():
    lib = _lib.load()
    info, target = _lib.UpsampleInfo(), _lib.PresentInfo(_lib.IMG_ACCUM, 0, 4, 4, 16, 0)
    lib.hrt_upsample_defaults(ctypes.byref(info), 4, 4)
    hits = np.zeros(16, dtype=_lib.HIT_DTYPE)
    dst = np.full(4 * 4 * 16, 7, np.uint8)
    ticket = ctypes.c_uint64(5)
    assert lib.hrt_upsample(None, ctypes.byref(info), None, None, _lib.ptr(hits), _lib.ptr(hits), _lib.FMT_RGBA32F,
                            _lib.ptr(dst), dst.nbytes) == 1
    assert lib.hrt_upsample_present(None, ctypes.byref(info), None, None, _lib.ptr(hits), _lib.ptr(hits),
                                    ctypes.byref(target), _lib.ptr(dst), dst.nbytes, ctypes.byref(ticket)) == 1
    assert lib.hrt_order_after(None, None) == 1
    assert (dst == 7).all() and ticket.value == 5  # nothing written
