"""Object motion in the temporal history on the CPU: the HIP-free coordinate header the
reprojection kernel and hrt_host_motion_between share (epq_raytracer_amd/csrc/hrt_motion_map.h), compiled into a
stand-alone program (tests/cpp/motion_map_test.cpp, -ffp-contract=off; once more under AddressSanitizer and UBSan),
against the numpy restatement tests/motion_ref.py word for word; then properties of the restatement itself -- static
tables are S15, co-motion is the identity -- hrt_host_motion_between, and the quality condition on CPU oracle frames."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import history_ref as H
import motion_ref as M
import epq_raytracer_amd as E
from epq_raytracer_amd import _lib
from helpers import SceneCase
from image_ref import same_floats
from test_history_ref import first_hits

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
F32 = np.float32
FLT_MAX = np.finfo(F32).max
EPS = 2.0 ** -24  # the unit roundoff of binary32


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def pose(r=None, t=(0, 0, 0)):
    r = np.eye(3) if r is None else r
    return np.concatenate([np.asarray(r, np.float64).T.reshape(9), np.asarray(t, np.float64)]).astype(F32)


def random_poses(rng, n):
    out = np.empty((n, 12), F32)
    for i in range(n):
        out[i] = pose(rotation(rng.normal(size=3), rng.uniform(-3.2, 3.2)), rng.uniform(-50, 50, 3))
    return out


# ---- the shared header ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["motion_map_test", "motion_map_test_san"])
def test_header_matches_the_restatement_bit_for_bit(target):
    subprocess.run(["make", "-s", "-C", CPP, "-f", "motion_demo.mk", target], check=True)
    rng = np.random.default_rng(21)
    n = 400
    rec = np.empty((n, 30), F32)
    rec[:, :12], rec[:, 12:24] = random_poses(rng, n), random_poses(rng, n)
    rec[:, 24:27] = rng.uniform(-100, 100, (n, 3))
    rec[:, 27:30] = rng.normal(size=(n, 3))
    rec[:20, 12:24] = rec[:20, :12]                       # equal poses
    rec[21, :12], rec[21, 12:24] = pose(None, (0.0, 0, 0)), pose(None, (-0.0, 0, 0))  # equal values, other bytes
    rec[22, 3], rec[23, 24], rec[24, 20] = np.nan, np.inf, FLT_MAX  # the arithmetic is defined for every float
    r = subprocess.run([os.path.join(CPP, target)], input=rec.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0 and b"ERROR" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:]
    got = np.frombuffer(r.stdout, np.uint32).reshape(n, 19)
    want = np.empty((n, 19), np.uint32)
    with np.errstate(all="ignore"):
        for i in range(n):
            g, flags = M.motion_between(rec[i, :12], rec[i, 12:24])
            tab = M.table([(g, M.MOVING)])
            p = [rec[i, 24 + k] for k in range(3)]
            nrm = [rec[i, 27 + k] for k in range(3)]
            pm = [((g[k] * p[0] + g[3 + k] * p[1]) + g[6 + k] * p[2]) + g[9 + k] for k in range(3)]
            nm = [(g[k] * nrm[0] + g[3 + k] * nrm[1]) + g[6 + k] * nrm[2] for k in range(3)]
            want[i, :12] = tab["m"][0].view(np.uint32)
            want[i, 12] = flags
            want[i, 13:16] = np.array(pm, F32).view(np.uint32)
            want[i, 16:19] = np.array(nm, F32).view(np.uint32)
    assert (want[:20, 12] == 0).all() and want[21, 12] == 1 and (want[25:, 12] == 1).all()
    same = (got == want) | (np.isnan(got.view(F32)) & np.isnan(want.view(F32)))
    assert same.all(), np.argwhere(~same)[:5]


# ---- hrt_host_motion_between ----------------------------------------------------------------------------------------

def test_host_motion_between_matches_the_restatement_and_maps_points_back():
    lib = _lib.load()
    rng = np.random.default_rng(4)
    prev, cur = random_poses(rng, 200), random_poses(rng, 200)
    worst = 0.0
    for a, b in zip(prev, cur):
        rec = E.motion_between(a, b)
        g, flags = M.motion_between(a, b)
        assert np.array(list(rec.m), F32).tobytes() == g.tobytes() and rec.flags == flags == M.MOVING
        assert list(rec.reserved) == [0, 0, 0]
        # A point the current pose places goes back to where the previous pose placed it.  In exact arithmetic on the
        # float32 poses, G (Rc x + tc) = Rp Rc^T Rc x + tp: tc cancels, and Rc^T Rc = I + E where Rc is a rotation
        # rounded entry by entry (each entry off by <= EPS, magnitude <= 1), so |E| <= 3 (2 EPS + EPS^2) < 6.1 EPS
        # per entry and |Rp E x| <= sqrt(3) * 3 * 6.1 EPS |x| < 32 EPS |x| per component (|.| the largest
        # component, sqrt(3) the largest absolute row sum of a rotation).  Rounding, with m = sqrt(3) |x| + |tc| the
        # bound of the placed point: L's entries carry <= 5 EPS each (3 products and 2 sums of terms <= 1), so L's
        # product with the placed point is off by <= 15 EPS m; the placed point's own rounding (<= 4 EPS m) goes
        # through L: <= 7 EPS m; b = tp - L tc is off by <= EPS |tp| + 3 * 8 EPS |tc|; G's application (3 products, 3
        # sums) adds <= 4 EPS (sqrt(3) m + |tp| + sqrt(3) |tc|).  Together below 82 EPS |x| + 61 EPS |tc| + 5 EPS |tp|;
        # the bound is 96 EPS (|x| + |tc| + |tp|).
        x = rng.uniform(-10, 10, 3).astype(F32)
        rp, tp, tc = a[:9].reshape(3, 3).T, a[9:], b[9:]
        with np.errstate(all="ignore"):
            world_cur = np.array([((b[k] * x[0] + b[3 + k] * x[1]) + b[6 + k] * x[2]) + b[9 + k] for k in range(3)], F32)
            back = np.array([((g[k] * world_cur[0] + g[3 + k] * world_cur[1]) + g[6 + k] * world_cur[2]) + g[9 + k]
                             for k in range(3)], F32)
        world_prev = rp.astype(np.float64) @ x.astype(np.float64) + tp.astype(np.float64)
        bound = 96 * EPS * float(np.abs(x).max() + np.abs(tp).max() + np.abs(tc).max())
        err = np.abs(back.astype(np.float64) - world_prev).max()
        worst = max(worst, err / bound)
        assert err <= bound, (err, bound)
    print(f"largest error / bound: {worst:.3f}")
    same = E.motion_between(prev[0], prev[0])
    assert same.flags == 0 and M.motion_between(prev[0], prev[0])[1] == 0
    out = _lib.Motion()
    fp = ctypes.POINTER(ctypes.c_float)
    lib.hrt_host_motion_between(None, prev[0].ctypes.data_as(fp), ctypes.byref(out))  # NULL arguments are ignored
    lib.hrt_host_motion_between(prev[0].ctypes.data_as(fp), prev[0].ctypes.data_as(fp), None)


# ---- properties of the restatement --------------------------------------------------------------------------------------

def synthetic(w, h, seed=3):
    from test_gpu_history import synthetic_guide, synthetic_source
    return synthetic_source(w, h, _lib.MODE_RGBA32F, seed), synthetic_guide(w, h, seed)


@pytest.mark.parametrize("filt", [H.NEAREST, H.BILINEAR])
@pytest.mark.parametrize("size", [(37, 23), (64, 64)])
def test_static_tables_are_s15(size, filt):
    from test_gpu_history import view_pairs
    w, h = size
    acc, hits = synthetic(w, h)
    prev_hits = hits.copy()
    prev_hits["kind"][::3, 1::4] = 0
    cnt = np.full((h, w), 9, np.uint32)
    still = M.table([(np.arange(12), 0)] * 9)
    for _, prev, cur in view_pairs(size)[:3]:
        want = H.reproject(acc, cnt, prev.record, prev_hits, cur.record, hits, filt)
        for spheres, meshes in ((None, None), (still, still), (still[:2], None)):
            got = M.reproject(acc, cnt, prev.record, prev_hits, cur.record, hits, spheres, meshes, filt)
            assert same_floats(got[0], want[0]).all() and np.array_equal(got[1], want[1])


@functools.lru_cache(maxsize=None)
def real_hits(name):
    case = SceneCase(name, (64, 64), num_samples=1, max_bounces=1)
    return case, first_hits(case)


@pytest.mark.parametrize("name", ["box", "spheres"])
def test_co_motion_is_the_identity(name):
    """The previous view is the current one carried along with every object, so the source coordinate is off the
    pixel's centre by rounding only: NEAREST returns A and N unchanged -- at every pixel under a translation, sky
    included (a miss looks along its direction, and the camera did not turn); at every pixel that has a hit under a
    rotation about a point."""
    case, hits = real_hits(name)
    h, w = hits.shape
    rng = np.random.default_rng(9)
    acc = rng.uniform(0, 4, (h, w, 4)).astype(F32)
    cnt = rng.integers(1, 40, (h, w)).astype(np.uint32)
    cur = E.View(case.camera, (w, h), case.settings).record
    n_s, n_m = len(case.spheres), len(case.meshes)

    def tables(g):
        return (M.table([(g, M.MOVING)] * n_s) if n_s else None), (M.table([(g, M.MOVING)] * n_m) if n_m else None)

    # a translation: the previous camera at o + b, every object's previous position at P + b
    b = np.array([0.5, -0.25, 2.0])
    prev = E.View(E.Camera([float(F32(c + d)) for c, d in zip(case.camera.position, b)], case.camera.direction,
                         case.camera.up), (w, h), case.settings).record
    got = M.reproject(acc, cnt, prev, hits, cur, hits, *tables(pose(None, b)), H.NEAREST)
    assert np.array_equal(got[1], cnt) and same_floats(got[0][..., :3], acc[..., :3]).all()
    # a rotation R about the point c: previous world = R (P - c) + c; the previous camera is the current one rotated
    # the same way, so in its frame nothing moved
    r = rotation([0.2, 1.0, -0.1], 0.4)
    c = np.array([0.3, 0.5, -0.2])
    pos = r @ (np.asarray(case.camera.position, np.float64) - c) + c
    prev_cam = E.Camera([float(F32(v)) for v in pos], [float(F32(v)) for v in r @ np.asarray(case.camera.direction, np.float64)],
                        [float(F32(v)) for v in r @ np.asarray(case.camera.up, np.float64)])
    # (the view matrix is built from direction and up, so it is R times the current one; the grid is the same in
    # camera space)
    prev = E.View(prev_cam, (w, h), case.settings).record
    prev_hits = hits.copy()
    prev_hits["normal"] = (np.asarray(hits["normal"], np.float64) @ r.T).astype(F32)
    got = M.reproject(acc, cnt, prev, prev_hits, cur, hits, *tables(pose(r, c - r @ c)), H.NEAREST, depth_tolerance=0.02,
                      min_normal_dot=0.9)
    hit = hits["kind"] != 0
    assert hit.sum() > 500
    assert np.array_equal(got[1][hit], cnt[hit]) and same_floats(got[0][hit][..., :3], acc[hit][..., :3]).all()


# ---- the quality condition, on CPU oracle frames ---------------------------------------------------------------------------

def test_following_the_mover_beats_ignoring_it_and_a_restart():
    """tools/motion_grid.py's row `box, sphere 0 by 0.47 along z` (about ten pixels): hrt_reproject rejects every pixel
    of the mover, so ignoring the motion is a restart there; following it keeps nine tenths of them, and after one new
    frame the error over the mover's pixels is a quarter of the restart's (DESIGN.md §36 has the whole table: 0.351
    against 1.434; the bound asked here is a half).  The rows the table shows lost -- a mirror sphere under the
    spheres scene's light, a featureless floor turned in its own plane -- are not asserted either way."""
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import motion_grid as G
    row = G.grid_row(*[m for m in G.MOVES if m[1] == "sphere 0 by 0.47 along z"][0])
    print(row)
    assert row["mover_pixels"] > 300 and row["kept_b"] == 0.0 and row["kept_a"] > 0.8
    a, b, c = (row["mse"][k] for k in "abc")
    assert b == c
    assert a[0] < 0.5 * c[0] and a[1] < c[1] and a[2] < c[2]
