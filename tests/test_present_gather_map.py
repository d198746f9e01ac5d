"""The gathered present's index arithmetic (epq_raytracer_amd/csrc/hrt_present_map.h: present_sx,
present_sy, gathered_row -- the functions hrt_image.hip's present kernels call), CPU only.  The test
compiles tests/cpp/present_map_test.cpp as plain C++ against the header, runs it over every case and
compares with the numpy sampling rule (tests/present_ref.py) and with the row-tile assembly of
epq_raytracer_amd/rowtiles.py; once more with the program built under ASan + UBSan."""
import json
import os
import subprocess

import numpy as np
import pytest

import present_ref
from epq_raytracer_amd import rowtiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "present_map_test.cpp")
INC = os.path.join(ROOT, "epq_raytracer_amd", "csrc")

SIZES = [(80, 70), (37, 23), (1, 130), (300, 1), (16384, 16384)]
PARTITIONS = [(2, 8), (3, 16), (8, 8), (5, 4), (3, 4), (1, None)]  # (parts, row_tile); one part: tile = height


def targets(ws, hs):
    if ws == 16384:  # the largest image: its own size and the single pixel (16384 -> 1)
        return [(ws, hs), (1, 1)]
    return [(ws, hs), (50, 31), (2 * ws, 2 * hs), (ws, max(hs // 2, 1)), (1, 1)]


def cases():
    out = []
    for ws, hs in SIZES:
        for parts, tile in PARTITIONS:
            tile = hs if tile is None else tile
            for wt, ht in targets(ws, hs):
                out.append((ws, hs, wt, ht, tile, parts, rowtiles.local_rows(hs, tile, parts)))
    return out


def build(tmp_path, extra=()):
    exe = str(tmp_path / ("present_map_test" + ("_san" if extra else "")))
    cmd = [os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-I", INC, *extra, SRC, "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def run(exe):
    args = [str(v) for c in cases() for v in c]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(line) for line in r.stdout.splitlines()]
    assert [tuple(d["case"]) for d in recs] == cases()
    return recs


def check(recs):
    index = {}  # (hs, tile, parts) -> assembly_index, global rows of every part
    for d in recs:
        ws, hs, wt, ht, tile, parts, local = d["case"]
        sx, sy = present_ref.source_index(ws, hs, wt, ht)
        assert np.array_equal(np.array(d["sx"], np.int64), sx), d["case"]
        assert np.array_equal(np.array(d["sy"], np.int64), sy), d["case"]
        if (hs, tile, parts) not in index:
            index[(hs, tile, parts)] = (rowtiles.assembly_index(hs, tile, parts),
                                        [rowtiles.global_rows(hs, tile, parts, p) for p in range(parts)])
        asm, glob = index[(hs, tile, parts)]
        grow = np.array(d["grow"], np.int64)
        # the row map is the inverse of the partition: gathered[assembly_index] is the full frame
        assert np.array_equal(grow, asm), d["case"]
        assert np.array_equal(np.array(d["trow"], np.int64), asm[sy]), d["case"]
        # 64-bit byte offsets (Python ints on this side)
        assert d["tbyte"] == [int(asm[s]) * ws * 16 for s in sy], d["case"]
        # whatever the library does: the rows reached below height lie inside the gather buffer, are
        # pairwise distinct, and none of them is a padded local row (a global row >= height)
        assert grow.min() >= 0 and grow.max() < parts * local, d["case"]
        assert len(np.unique(grow)) == hs, d["case"]
        back = np.array([glob[r // local][r % local] for r in grow])
        assert np.array_equal(back, np.arange(hs)), d["case"]
        assert (back < hs).all()


def test_map_matches_numpy_rule_and_row_tiles(tmp_path):
    exe, r = build(tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = run(exe)
    assert len(recs) == len(SIZES) * len(PARTITIONS) * 5 - len(PARTITIONS) * 3
    # the largest case does pass 2^32 bytes (what the 64-bit row offset is for)
    assert max(max(d["tbyte"]) for d in recs) >= 1 << 32
    check(recs)


def test_map_under_sanitizers(tmp_path):
    """The same program as a stand-alone ASan + UBSan binary: no overflow, no out-of-range shift or
    conversion reported over every case, and the same output."""
    exe, r = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    if r.returncode != 0:
        pytest.skip("the toolchain cannot link the sanitizer runtimes: " + r.stderr[-300:])
    check(run(exe))
