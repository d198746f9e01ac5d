"""Ray queries on the CPU: the layouts of hrt_ray_query / hrt_hit / hrt_query_stats (a compiled C probe
against the ctypes mirrors), the exports, the NULL-handle rejection, and the reference of the GPU suite
(tests/query_ref.py): its exact fused multiply-add and its restated triangle test against the oracle."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np

import pyoracle
import query_ref as Q
from epq_raytracer_amd import _lib
from helpers import SceneCase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_FIELDS = ("origin", "t_max", "direction", "reserved")
HIT_FIELDS = ("t", "kind", "index", "mesh", "normal", "reserved")
STATS_FIELDS = ("method_ran", "reserved", "scan_rays", "tri_tests")
FLT_MAX = Q.FLT_MAX


def test_struct_layouts(tmp_path):
    recs = (("hrt_ray_query", RAY_FIELDS), ("hrt_hit", HIT_FIELDS), ("hrt_query_stats", STATS_FIELDS))
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d %d %d %d %u\\n", sizeof(hrt_ray_query), sizeof(hrt_hit),\n'
                   '         sizeof(hrt_query_stats), (int)HRT_QUERY_AUTO, (int)HRT_QUERY_SCAN, (int)HRT_QUERY_BVH,\n'
                   '         (int)HRT_QUERY_PAIRS, HRT_ABI_VERSION);\n'
                   + "".join(f'  printf("%zu\\n", offsetof({r}, {f}));\n' for r, fs in recs for f in fs)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:8] == [32, 32, 24, 0, 1, 2, 3, 6]  # additive: the ABI version stays 6
    assert (_lib.QUERY_AUTO, _lib.QUERY_SCAN, _lib.QUERY_BVH, _lib.QUERY_PAIRS, _lib.ABI_VERSION) == (0, 1, 2, 3, 6)
    at = 8
    for cls, dtype, fields, want in ((_lib.RayQuery, _lib.RAY_QUERY_DTYPE, RAY_FIELDS, [0, 12, 16, 28]),
                                     (_lib.Hit, _lib.HIT_DTYPE, HIT_FIELDS, [0, 4, 8, 12, 16, 28]),
                                     (_lib.QueryStats, None, STATS_FIELDS, [0, 4, 8, 16])):
        assert [n for n, _ in cls._fields_] == list(fields)
        assert [getattr(cls, f).offset for f in fields] == out[at:at + len(fields)] == want
        if dtype is not None:
            assert dtype.names == fields and [dtype.fields[f][1] for f in fields] == want
            assert dtype.itemsize == ctypes.sizeof(cls)
        at += len(fields)
    assert ctypes.sizeof(_lib.RayQuery) == 32 and ctypes.sizeof(_lib.Hit) == 32 and ctypes.sizeof(_lib.QueryStats) == 24


def test_symbols_exported_from_both_libraries():
    names = {"hrt_intersect", "hrt_intersect_primary"}
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
        assert names <= exported, path
    assert names <= set(_lib.EXPORTED_SYMBOLS)
    for lib in (_lib.load(), _lib.load(debug=True)):
        assert lib.hrt_intersect.argtypes and lib.hrt_intersect_primary.argtypes


def test_null_handles_are_rejected():
    lib = _lib.load()
    rays = np.zeros(2, _lib.RAY_QUERY_DTYPE)
    hits = np.full(2, 7, np.uint8).repeat(32).view(_lib.HIT_DTYPE)
    before = hits.tobytes()
    st = _lib.QueryStats(9, 9, 9, 9)
    assert lib.hrt_intersect(None, _lib.ptr(rays), 2, _lib.QUERY_SCAN, _lib.ptr(hits), ctypes.byref(st)) == 1
    pc = _lib.PushConstants()
    assert lib.hrt_intersect_primary(None, ctypes.byref(pc), 0, 0, 1, 1, _lib.QUERY_SCAN, _lib.ptr(hits),
                                     ctypes.byref(st)) == 1
    assert hits.tobytes() == before and (st.method_ran, st.scan_rays, st.tri_tests) == (9, 9, 9)  # nothing written


def test_exact_fma_rounds_once():
    f = np.float32
    # ties and near-ties of the single rounding
    a, b, c = f(1 + 2.0 ** -12), f(1 + 2.0 ** -12), f(-(2.0 ** -11))  # exact: 1 + 2^-24
    assert Q.fma32(a, b, c) == f(1.0)  # the tie goes to even
    assert Q.fma32(f(1 + 2.0 ** -12), f(1 + 2.0 ** -12), f(-(2.0 ** -11) + 2.0 ** -35)) == np.nextafter(f(1.0), f(2))
    # zeros, denormals, overflow, non-finite operands
    assert math.copysign(1, Q.fma32(f(-0.0), f(1.0), f(-0.0))) == -1 and Q.fma32(f(-0.0), f(1.0), f(-0.0)) == 0
    assert math.copysign(1, Q.fma32(f(-0.0), f(1.0), f(0.0))) == 1
    assert math.copysign(1, Q.fma32(f(1.0), f(-1.0), f(1.0))) == 1  # exact cancellation: +0
    assert Q.fma32(f(2.0 ** -100), f(2.0 ** -49), f(0)) == f(2.0 ** -149)
    assert Q.fma32(f(2.0 ** -100), f(2.0 ** -50), f(0)) == 0  # the tie at half the smallest denormal: even
    assert Q.fma32(f(3e38), f(2.0), f(0)) == f(np.inf) and Q.fma32(f(3e38), f(2.0), f(-3e38)) == f(3e38)
    assert np.isnan(Q.fma32(f(np.inf), f(0.0), f(1.0))) and Q.fma32(f(np.inf), f(1.0), f(1.0)) == f(np.inf)
    # against exact rational arithmetic on random operands of mixed magnitude
    rng = np.random.default_rng(21)
    for _ in range(400):
        x, y, z = (f(rng.normal() * 10.0 ** rng.integers(-12, 12)) for _ in range(3))
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        got = Fraction(float(Q.fma32(x, y, z)))
        lo, hi = float(np.nextafter(f(float(got)), f(-np.inf))), float(np.nextafter(f(float(got)), f(np.inf)))
        assert abs(got - exact) <= abs(Fraction(lo) - exact) and abs(got - exact) <= abs(Fraction(hi) - exact)


def _tri(a, b, c):
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    t = np.zeros((), dtype=_lib.TRIANGLE_DTYPE)
    e1, e2 = b - a, c - a
    n = np.float32([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    t["a"][:3], t["edge_one"][:3], t["edge_two"][:3], t["normal"][:3] = a, e1, e2, n
    return t


def test_restated_triangle_test_matches_the_oracle():
    """query_ref's intersecting_tri (exact fma) gives the oracle's distance: the analytic known answers of
    tests/test_oracle.py, then the bits on random rays against the box scene's triangles."""
    t = _tri([0, 0, 0], [1, 0, 0], [0, 1, 0])
    kats = (([0.25, 0.25, 1], [0, 0, -1], 1.0), ([0.25, 0.25, -1], [0, 0, 1], FLT_MAX), ([2, 2, 1], [0, 0, -1], FLT_MAX),
            ([0.25, 0.25, -1], [0, 0, -1], FLT_MAX), ([0.0, 0.5, 2], [0, 0, -1], 2.0), ([0.0, 0.0, 2], [0, 0, -1], 2.0),
            ([-1, 0.25, 0], [1, 0, 0], FLT_MAX))
    for o, d, want in kats:
        o, d = np.float32(o), np.float32(d)
        assert Q.tri_dist32(t, o, d) == np.float32(want) == pyoracle.intersecting_tri(t, o, d)[3]
    assert Q.tri_dist32(_tri([0, 0, 0], [4, 0, 0], [0, 4, 0]), np.float32([1, 1, 3]), np.float32([0, 0, -1])) == 3.0
    case = SceneCase("box", (8, 8), 1, 1)
    qs = Q.QueryScene(case)
    rays = np.concatenate([Q.family(qs, n, 12, 3, case.push()) for n in "abcdef"])
    hits = 0
    for r in rays:
        d, _ = Q.normalize32(r["direction"])
        for tri in case.tris:
            want = pyoracle.intersecting_tri(tri, r["origin"], d)[3]
            got = Q.tri_dist32(tri, r["origin"], d)
            assert got.tobytes() == np.float32(want).tobytes(), (r, tri)
            hits += int(want != FLT_MAX)
    assert hits > 50


def test_reference_world_hit_basics():
    """The reference's own rules: certain misses, t_max as a strict bound, the scan fallback's rays."""
    case = SceneCase("box", (8, 8), 1, 1)
    qs = Q.QueryScene(case)
    pr = Q.primary_rays(case, case.push(), [4], [4])[0]
    t, kind, idx, mesh, nrm, tests, scan = qs.world_hit(pr["origin"], pr["direction"])
    assert kind in (1, 2) and t < FLT_MAX and tests > 0 and not scan
    assert qs.world_hit(pr["origin"], pr["direction"], t)[1] == 0  # strict: dist < t_max
    assert qs.world_hit(pr["origin"], pr["direction"], np.nextafter(t, np.float32(np.inf)))[:3] == (t, kind, idx)
    for bad in (np.nan, -1.0, 0.001, 0.0):
        assert qs.world_hit(pr["origin"], pr["direction"], bad)[:2] == (FLT_MAX, 0)
        assert qs.world_hit(pr["origin"], pr["direction"], bad)[5:] == (0, False)
    assert qs.world_hit(pr["origin"], [0, 0, 0])[6] and qs.world_hit([np.nan, 0, 0], pr["direction"])[6]
    h = Q.family(qs, "h", 64, 5)
    assert 0 < Q.count_irregular(h) < 64
    assert Q.count_irregular(np.concatenate([Q.family(qs, n, 16, 5, case.push()) for n in "abcdef"])) == 0
