"""Tile-masked refinement on the CPU: the layout of hrt_refine_tiles_stats (a compiled C probe against the ctypes
mirror), the constant, the exports of both libraries, the kernels in the code object and the NULL-handle rejection."""
import ctypes
import os
import subprocess

import numpy as np

from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("kernel_ran", "whole_frame", "tiles", "tiles_selected", "items", "reserved", "selected", "pixels_traced")
NAMES = {"hrt_refine_tiles", "hrt_refine_tiles_until"}


def test_struct_layout_and_constant(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %u %u\\n", sizeof(hrt_refine_tiles_stats), HRT_REFINE_TILES_MAX_FRAMES, HRT_ABI_VERSION);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_refine_tiles_stats, {f}));\n' for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [40, 4096, 6]  # additive: the ABI version stays 6
    offsets = [0, 4, 8, 12, 16, 20, 24, 32]
    assert out[3:] == offsets
    assert [n for n, _ in _lib.RefineTilesStats._fields_] == list(FIELDS)
    assert [getattr(_lib.RefineTilesStats, f).offset for f in FIELDS] == offsets
    assert ctypes.sizeof(_lib.RefineTilesStats) == 40 and _lib.REFINE_TILES_MAX_FRAMES == 4096
    # hrt_refine's methods did not grow
    assert set(_lib.REFINE_NAMES) == {0, 1, 2} and _lib.ABI_VERSION == 6


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
    # Itanium mangling: refine_fold_frames<T, Moments> (j: uint32_t)
    for k in (b"_ZN3hrt16refine_tile_bitsE", b"_ZN3hrt16plan_hist_maskedE", b"_ZN3hrt16plan_fill_maskedE",
              b"refine_fold_framesIjLb0E", b"refine_fold_framesIjLb1E"):
        assert k in blob, k
    k = b"refine_fold_framesI15HIP_vector_typeIfLj4EELb"
    assert k + b"0E" in blob and k + b"1E" in blob
    # the whole-frame planner the masked one restates, and the fold it extends, are still there
    assert b"_ZN3hrt9plan_histE" in blob and b"_ZN3hrt9plan_scanE" in blob and b"_ZN3hrt9plan_fillE" in blob
    assert b"refine_fold_imageIjLb1E" in blob


def test_null_handles_are_rejected():
    lib = _lib.load()
    rule, pc, stats = _lib.RefineRule(), _lib.PushConstants(), _lib.RefineTilesStats()
    lib.hrt_refine_defaults(ctypes.byref(rule))
    mask = np.full(16, 7, np.uint32)
    passes, frames, settled = ctypes.c_uint32(5), ctypes.c_uint64(5), ctypes.c_uint32(5)
    assert lib.hrt_refine_tiles(None, ctypes.byref(pc), _lib.ptr(mask), 8, 1, 0, ctypes.byref(stats)) == 1
    assert lib.hrt_refine_tiles_until(None, ctypes.byref(pc), ctypes.byref(rule), None, 8, 4, 1, 0, ctypes.byref(passes),
                                      ctypes.byref(frames), ctypes.byref(settled)) == 1
    assert (mask == 7).all() and (passes.value, frames.value, settled.value) == (5, 5, 5)  # nothing written
    assert bytes(stats) == bytes(40)
