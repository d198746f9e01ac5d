"""Adaptive refinement on the CPU: the layouts of hrt_refine_rule and hrt_refine_stats (a compiled C probe against the
ctypes mirrors), the constants, the exports of both libraries, the kernels in the code object, hrt_refine_defaults and
the NULL-handle rejection."""
import ctypes
import os
import subprocess

import numpy as np

import refine_ref as R
from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE_FIELDS = ("min_history", "max_count", "radius", "flags", "tolerance", "luminance_floor", "reserved")
STATS_FIELDS = ("method_ran", "query_method_ran", "selected", "scan_segments", "segments", "tri_tests", "reserved")
NAMES = {"hrt_refine_defaults", "hrt_refine_select", "hrt_refine", "hrt_refine_until"}


def test_struct_layouts_and_constants(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %zu %d %d %d %u %u %u %u %u %u\\n", sizeof(hrt_refine_rule), sizeof(hrt_refine_stats),\n'
                   '         (int)HRT_REFINE_AUTO, (int)HRT_REFINE_QUERIES, (int)HRT_REFINE_FRAME, HRT_REFINE_MOMENTS,\n'
                   '         HRT_REFINE_MIN_HISTORY, HRT_REFINE_MAX_COUNT, HRT_REFINE_RADIUS, HRT_REFINE_MAX_RADIUS,\n'
                   '         HRT_ABI_VERSION);\n'
                   '  printf("%.9g %.9g\\n", (double)HRT_REFINE_TOLERANCE, (double)HRT_REFINE_FLOOR);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_refine_rule, {f}));\n' for f in RULE_FIELDS)
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_refine_stats, {f}));\n' for f in STATS_FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    # additive: the ABI version stays 6
    assert [int(v) for v in out[:11]] == [32, 48, 0, 1, 2, 1, 4, 1 << 24, 1, 3, 6]
    assert tuple(float(np.float32(v)) for v in out[11:13]) == (float(np.float32(0.05)), float(np.float32(0.01)))
    rule_off, stats_off = [0, 4, 8, 12, 16, 20, 24], [0, 4, 8, 16, 24, 32, 40]
    assert [int(v) for v in out[13:20]] == rule_off and [int(v) for v in out[20:]] == stats_off
    assert [n for n, _ in _lib.RefineRule._fields_] == list(RULE_FIELDS)
    assert [n for n, _ in _lib.RefineStats._fields_] == list(STATS_FIELDS)
    assert [getattr(_lib.RefineRule, f).offset for f in RULE_FIELDS] == rule_off and ctypes.sizeof(_lib.RefineRule) == 32
    assert [getattr(_lib.RefineStats, f).offset for f in STATS_FIELDS] == stats_off and ctypes.sizeof(_lib.RefineStats) == 48
    assert (_lib.REFINE_AUTO, _lib.REFINE_QUERIES, _lib.REFINE_FRAME, _lib.REFINE_MOMENTS) == (0, 1, 2, 1)
    assert set(_lib.REFINE_NAMES) == {0, 1, 2} and _lib.REFINE_MAX_RADIUS == 3
    assert R.DEFAULTS == (_lib.REFINE_MIN_HISTORY, _lib.REFINE_MAX_COUNT, _lib.REFINE_RADIUS, _lib.REFINE_TOLERANCE,
                          _lib.REFINE_FLOOR) == (4, 1 << 24, 1, 0.05, 0.01)
    assert _lib.REFINE_MAX_COUNT == _lib.HISTORY_MAX and _lib.ABI_VERSION == 6


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
    # Itanium mangling: refine_select<Guided>, refine_queries<Emit>, refine_fold[_image]<T, Moments> (j: uint32_t)
    for k in (b"refine_selectILb0E", b"refine_selectILb1E", b"refine_queriesILb0E", b"refine_queriesILb1E",
              b"refine_foldIjLb0E", b"refine_foldIjLb1E", b"refine_fold_imageIjLb0E", b"refine_fold_imageIjLb1E"):
        assert k in blob, k
    for k in (b"refine_foldI15HIP_vector_typeIfLj4EELb", b"refine_fold_imageI15HIP_vector_typeIfLj4EELb"):
        assert k + b"0E" in blob and k + b"1E" in blob, k
    # the history folds the refinement shares its device functions with are still there
    assert b"fold_history_moments" in blob and b"fold_historyIj" in blob


def test_defaults():
    for lib in (_lib.load(), _lib.load(debug=True)):
        rule = _lib.RefineRule(9, 9, 9, 9, -1.0, -1.0, (7, 7))
        lib.hrt_refine_defaults(ctypes.byref(rule))
        assert (rule.min_history, rule.max_count, rule.radius, rule.flags) == R.DEFAULTS[:3] + (0,)
        assert (rule.tolerance, rule.luminance_floor) == tuple(float(np.float32(v)) for v in R.DEFAULTS[3:])
        assert tuple(rule.reserved) == (0, 0)
        lib.hrt_refine_defaults(None)  # ignored


def test_null_handles_are_rejected():
    lib = _lib.load()
    rule, pc, stats = _lib.RefineRule(), _lib.PushConstants(), _lib.RefineStats()
    lib.hrt_refine_defaults(ctypes.byref(rule))
    mask = np.full(16, 7, np.uint32)
    n, passes, frames, settled = ctypes.c_uint64(5), ctypes.c_uint32(5), ctypes.c_uint64(5), ctypes.c_uint32(5)
    assert lib.hrt_refine_select(None, ctypes.byref(rule), None, _lib.ptr(mask), ctypes.byref(n)) == 1
    assert lib.hrt_refine(None, ctypes.byref(pc), _lib.ptr(mask), 8, 0, 0, 0, ctypes.byref(stats)) == 1
    assert lib.hrt_refine_until(None, ctypes.byref(pc), ctypes.byref(rule), None, 8, 4, 0, 0, ctypes.byref(passes),
                                ctypes.byref(frames), ctypes.byref(settled)) == 1
    assert (mask == 7).all() and (n.value, passes.value, frames.value, settled.value) == (5, 5, 5, 5)  # nothing written
