"""Fold records and hrt_compute_until on the CPU: the layouts of hrt_fold_record / hrt_settle_rule (a
compiled C probe against the ctypes mirrors), the exports, the freeze frame of the 8-bit accumulator
(HRT_RGBA8_FREEZE_FRAME, derived here from the oracle's combiner over every channel pair), and the
settle rule of tests/fold_ref.py -- its properties, and its stop frames on the oracle's own island
frames, which pin the inputs of tests/test_gpu_fold_records.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

import fold_ref
import pyoracle
from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hip_raytrace.h")
RECORD_FIELDS = ("frame", "changed_pixels", "max_delta", "reserved", "abs_delta_sum")
RULE_FIELDS = ("max_changed_pixels", "max_delta", "quiet_frames", "flags")


def header_define(name: str) -> int:
    m = re.search(rf"#define {name}\s+(\d+)u?\b", open(HEADER).read())
    assert m, name
    return int(m.group(1))


def test_struct_layouts(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %zu %d %u %u\\n", sizeof(hrt_fold_record), sizeof(hrt_settle_rule),\n'
                   '         (int)HRT_OPT_FOLD_RECORDS, HRT_FOLD_RECORD_RING, HRT_RGBA8_FREEZE_FRAME);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_fold_record, {f}));\n' for f in RECORD_FIELDS)
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_settle_rule, {f}));\n' for f in RULE_FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:5] == [24, 16, 19, 1024, 510]
    assert (_lib.OPT_FOLD_RECORDS, _lib.FOLD_RECORD_RING, _lib.RGBA8_FREEZE_FRAME) == (19, 1024, 510)
    assert ctypes.sizeof(_lib.FoldRecord) == 24 and ctypes.sizeof(_lib.SettleRule) == 16
    assert [n for n, _ in _lib.FoldRecord._fields_] == list(RECORD_FIELDS)
    assert [n for n, _ in _lib.SettleRule._fields_] == list(RULE_FIELDS)
    assert [getattr(_lib.FoldRecord, f).offset for f in RECORD_FIELDS] == out[5:10] == [0, 4, 8, 12, 16]
    assert [getattr(_lib.SettleRule, f).offset for f in RULE_FIELDS] == out[10:14] == [0, 4, 8, 12]
    assert _lib.FoldRecord.abs_delta_sum.size == 8
    # the structured dtype HrtContext.fold_records returns
    assert _lib.FOLD_RECORD_DTYPE.itemsize == 24 and _lib.FOLD_RECORD_DTYPE.names == RECORD_FIELDS
    assert [_lib.FOLD_RECORD_DTYPE.fields[f][1] for f in RECORD_FIELDS] == out[5:10]


def test_symbols_exported_from_both_libraries():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
        assert {"hrt_get_fold_records", "hrt_compute_until"} <= exported, path
    assert {"hrt_get_fold_records", "hrt_compute_until"} <= set(_lib.EXPORTED_SYMBOLS)
    for lib in (_lib.load(), _lib.load(debug=True)):
        assert lib.hrt_get_fold_records.argtypes and lib.hrt_compute_until.argtypes


def test_null_handles_are_rejected():
    lib = _lib.load()
    pc, rule = _lib.PushConstants(), _lib.SettleRule(0, 0, 1, 0)
    done, settled, count, total = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint64(7)
    assert lib.hrt_compute_until(None, ctypes.byref(pc), 4, ctypes.byref(rule), ctypes.byref(done),
                                 ctypes.byref(settled)) == 1
    assert lib.hrt_get_fold_records(None, None, 0, ctypes.byref(count), ctypes.byref(total)) == 1
    assert (done.value, settled.value, count.value, total.value) == (7, 7, 7, 7)  # nothing written


def test_rgba8_accumulator_freezes():
    """image_combiner.glsl's 8-bit fold over all 65,536 (previous, new) channel values, frames 1..1199 (the
    oracle's combiner): some pair still changes at frame 509, none at any frame >= HRT_RGBA8_FREEZE_FRAME --
    from there the fold is the identity on the accumulator whatever the new frame holds."""
    freeze = header_define("HRT_RGBA8_FREEZE_FRAME")
    assert freeze == 510
    prev = np.zeros((256, 256, 4), np.uint8)
    prev[..., :3] = np.arange(256, dtype=np.uint8)[:, None, None]
    prev[..., 3] = 255
    new = np.zeros((256, 256, 4), np.uint8)
    new[..., :3] = np.arange(256, dtype=np.uint8)[None, :, None]
    new[..., 3] = 255
    last_change = 0
    for frame in range(1, 1200):
        cur = prev.copy()
        pyoracle.accumulate_rgba8(frame, cur, new)
        if (cur != prev).any():
            last_change = frame
        assert frame < freeze or (cur == prev).all(), frame
    assert last_change == freeze - 1 == 509


def test_stop_frame_properties():
    q, loud = (0, 0, 0), (50, 500, 30)
    # a run broken by one loud frame restarts
    assert fold_ref.stop_frame([q, q, loud, q, q, q], 6, 0, 0, 3) == (6, True)
    assert fold_ref.stop_frame([q, q, loud, q, q, q], 5, 0, 0, 3) == (5, False)
    assert fold_ref.stop_frame([q, q, q, loud], 4, 0, 0, 3) == (3, True)
    assert fold_ref.stop_frame([loud, q], 2, 0, 0, 1) == (2, True)
    # quiet_frames > max_frames never settles
    assert fold_ref.stop_frame([q] * 8, 4, 0, 0, 5) == (4, False)
    assert fold_ref.stop_frame([q] * 8, 5, 0, 0, 5) == (5, True)
    # the two bounds combine with AND; 0xFFFFFFFF disables one
    few_big, many_small = (3, 90, 40), (900, 900, 1)
    assert not fold_ref.quiet(few_big, 10, 8) and not fold_ref.quiet(many_small, 10, 8)
    assert fold_ref.quiet(few_big, 10, fold_ref.ANY) and fold_ref.quiet(many_small, fold_ref.ANY, 8)
    assert fold_ref.quiet((10, 80, 8), 10, 8) and not fold_ref.quiet((11, 80, 8), 10, 8)
    assert fold_ref.stop_frame([few_big, many_small, (10, 80, 8)], 3, 10, 8, 1) == (3, True)
    assert fold_ref.stop_frame([loud] * 3, 3) == (1, True)  # no bound at all: the first frame is quiet
    assert fold_ref.stop_frame([], 0) == (0, False)
    # records of a fold
    a = np.zeros((2, 3, 4), np.uint8)
    b = a.copy()
    b[0, 1] = (5, 0, 250, 0)
    b[1, 2, 3] = 1
    assert fold_ref.records(a, b) == (2, 256, 250) and fold_ref.records(b, a) == (2, 256, 250)
    assert fold_ref.records(a, a) == (0, 0, 0)


def test_island_oracle_stop_frames():
    """The stop frames the GPU cases rely on, from the oracle's own frames: 23 under {1000 changed pixels,
    any delta, 2 quiet frames} and 18 under {any, delta 12, 3}."""
    recs = fold_ref.oracle_records("island", (96, 64), 3, 8, 24)
    assert all(r[0] >= 6000 for r in recs[:21]) and [r[0] for r in recs[21:]] == [593, 583, 577]
    assert (recs[0][2], recs[15][2], recs[23][2]) == (128, 12, 7)
    assert fold_ref.stop_frame(recs, 24, 1000, fold_ref.ANY, 2) == (23, True)
    assert fold_ref.stop_frame(recs, 24, fold_ref.ANY, 12, 3) == (18, True)
