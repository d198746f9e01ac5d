"""The present pass on the CPU: hrt_present_info's layout (a compiled C probe against the ctypes
mirror) and the properties of the pinned sampling rule that tests/test_gpu_present.py builds every
expected target from (tests/present_ref.py)."""
import ctypes
import os
import random
import subprocess

import numpy as np

import present_ref
from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("image_id", "format", "width", "height", "pitch", "flags")


def test_present_info_layout(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %d %d\\n", sizeof(hrt_present_info), HRT_PRESENT_B8G8R8A8, HRT_PRESENT_R8G8B8A8);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_present_info, {f}));\n' for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:3]] == [24, _lib.PRESENT_B8G8R8A8, _lib.PRESENT_R8G8B8A8]
    assert ctypes.sizeof(_lib.PresentInfo) == 24
    assert [name for name, _ in _lib.PresentInfo._fields_] == list(FIELDS)
    assert [getattr(_lib.PresentInfo, f).offset for f in FIELDS] == [int(v) for v in out[3:]]
    assert all(getattr(_lib.PresentInfo, f).size == 4 for f in FIELDS)
    assert (present_ref.B8G8R8A8, present_ref.R8G8B8A8) == (_lib.PRESENT_B8G8R8A8, _lib.PRESENT_R8G8B8A8)


def test_present_entry_points_bound():
    lib = _lib.load()
    for name in ("hrt_present", "hrt_accumulate_present", "hrt_present_done", "hrt_present_wait"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name).argtypes
    # no context: rejected before anything else is looked at
    info, t = _lib.PresentInfo(_lib.IMG_ACCUM, 0, 1, 1, 4, 0), ctypes.c_uint64()
    assert lib.hrt_present(None, ctypes.byref(info), None, 4, ctypes.byref(t)) == 1
    assert lib.hrt_accumulate_present(None, 0, ctypes.byref(info), None, 4, ctypes.byref(t)) == 1
    assert lib.hrt_present_done(None, 1, None) == 1 and lib.hrt_present_wait(None, 1) == 1


def test_sampling_rule_properties():
    """1,000 random size pairs: indices in range, sx monotone in x, sy anti-monotone in y, and at equal
    sizes the identity in x and the flip in y."""
    rng = random.Random(20240611)
    for k in range(1000):
        ws, hs, wt, ht = (rng.randint(1, 300) for _ in range(4))
        if k % 4 == 0:
            wt, ht = ws, hs
        elif k % 4 == 1:  # up to the largest target and a source beyond 2^16: the products need 64 bits
            ws, wt = rng.randint(1, 1 << 20), rng.choice((1, 16383, 16384))
        sx, sy = present_ref.source_index(ws, hs, wt, ht)
        assert len(sx) == wt and len(sy) == ht
        assert sx.min() >= 0 and sx.max() < ws and sy.min() >= 0 and sy.max() < hs
        assert (np.diff(sx) >= 0).all() and (np.diff(sy) <= 0).all()
        if (wt, ht) == (ws, hs):
            assert (sx == np.arange(ws)).all() and (sy == hs - 1 - np.arange(hs)).all()


def test_sampling_rule_texel_edges():
    """A sample exactly on a texel edge (source twice the target) takes the texel that starts at the edge
    (the floor of the unflipped coordinate): the pin of DESIGN.md §2."""
    sx, sy = present_ref.source_index(64, 48, 32, 24)
    assert (sx == 2 * np.arange(32) + 1).all()
    assert (sy == 48 - 1 - (2 * np.arange(24) + 1)).all()


def test_reference_target_bytes():
    src = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    raw = present_ref.present_bytes(src, 3, 2, 16, present_ref.B8G8R8A8, 40, offset=4)
    assert (raw[:4] == 0xA5).all() and (raw[16:20] == 0xA5).all() and (raw[32:] == 0xA5).all()
    assert raw[4:16].tolist() == [14, 13, 12, 15, 18, 17, 16, 19, 22, 21, 20, 23]  # the source's last row, BGRA
    assert raw[20:32].tolist() == [2, 1, 0, 3, 6, 5, 4, 7, 10, 9, 8, 11]
    same = present_ref.present_pixels(src, 3, 2, present_ref.R8G8B8A8)
    assert (same == src[::-1]).all()
