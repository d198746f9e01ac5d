"""The temporal history's numpy reference (tests/history_ref.py) on the CPU: the properties S15
implies, and the quality condition of the default thresholds on oracle frames -- after a camera move, history
carried across by the reprojection is closer to the oracle's 256-frame accumulation in the new view than a
restart at the move, after 1, 2 and 4 new frames (DESIGN.md §28 has the grid the defaults come from)."""
import copy
import functools

import numpy as np
import pytest

import history_ref as H
import image_ref as I
import pyoracle
import query_ref as Q
import epq_raytracer_amd as E
from epq_raytracer_amd import _lib
from helpers import SceneCase
from image_ref import same_floats

F32 = np.float32
FLT_MAX = np.finfo(F32).max
SIZE = (64, 64)
# The move of the quality condition: a translation and a turn of 0.08 of the focal length sideways and 0.03 up --
# 2 to 3 pixels across and 1 to 2 down at 64 x 64 (the median of S15's u - x and w - y on both scenes).
MOVE_POSITION, MOVE_TURN = (0.06, 0.03, 0.04), (0.08, 0.03)


def moved(cam, dpos=MOVE_POSITION, turn=MOVE_TURN):
    d = np.asarray(cam.direction, np.float64)
    d /= np.linalg.norm(d)
    up = np.asarray(cam.up, np.float64)
    side = np.cross(d, up)
    side /= np.linalg.norm(side)
    nd = d + turn[0] * side + turn[1] * up
    return E.Camera([float(F32(a + b)) for a, b in zip(cam.position, dpos)], [float(F32(v)) for v in nd], cam.up)


def make_hits(h, w, kind=0, mesh=_lib.HIT_NONE, index=_lib.HIT_NONE, t=FLT_MAX, normal=(0.0, 0.0, 0.0)):
    hits = np.zeros((h, w), dtype=_lib.HIT_DTYPE)
    hits["kind"], hits["mesh"], hits["index"], hits["t"], hits["normal"] = kind, mesh, index, t, normal
    return hits


def first_hits(case):
    w, h = case.size
    ys, xs = np.mgrid[0:h, 0:w]
    return Q.QueryScene(case).hits(Q.primary_rays(case, case.push(), xs.reshape(-1), ys.reshape(-1)))[0].reshape(h, w)


@functools.lru_cache(maxsize=None)
def oracle_move(name):
    """A 64 x 64 RGBA32F render (1 spp, 8 bounces) before and after the move: the two views and their first hits,
    16 frames of the old view, 4 of the new one and the oracle's accumulation of 256 other frames of the new."""
    prev = SceneCase(name, SIZE, num_samples=1, max_bounces=8)
    cur = SceneCase(name, SIZE, num_samples=1, max_bounces=8)
    cur.camera = moved(prev.camera)
    views = tuple(E.View(c.camera, SIZE, c.settings).record for c in (prev, cur))
    old = [prev.oracle(rng_offset=1 + k, want_f32=True)[1] for k in range(16)]
    new = [cur.oracle(rng_offset=1000 + k, want_f32=True)[1] for k in range(4)]
    target = np.zeros(SIZE[::-1] + (4,), F32)
    for k in range(256):
        pyoracle.accumulate_rgba32f(k, target, cur.oracle(rng_offset=2000 + k, want_f32=True)[1])
    return views, (first_hits(prev), first_hits(cur)), old, new, target


def history_of(frames, max_history=32):
    acc, cnt = np.zeros_like(frames[0]), np.zeros(frames[0].shape[:2], np.uint32)
    for f in frames:
        acc, cnt = H.accumulate_history(acc, cnt, f, max_history)
    return acc, cnt


def random_image(rng, h, w, dtype):
    if dtype == np.uint8:
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return rng.uniform(0, 4, (h, w, 4)).astype(F32)


@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_fold_is_the_combiner_at_the_pixels_own_frame_number(dtype):
    rng = np.random.default_rng(5)
    h, w = 6, 9
    acc, new = random_image(rng, h, w, dtype), random_image(rng, h, w, dtype)
    cnt = rng.integers(0, 5, (h, w)).astype(np.uint32)
    cnt[0, :4] = [1 << 24, (1 << 24) - 1, 31, 32]
    out, nxt = H.accumulate_history(acc, cnt, new, 32)
    fold = I.fold_rgba8 if dtype == np.uint8 else I.fold_rgba32f
    for y in range(h):
        for x in range(w):
            n = int(cnt[y, x])
            if n == 0:  # the new texel alone, with the accumulator's alpha
                want = new[y, x].copy()
                want[3] = 255 if dtype == np.uint8 else 1.0
            else:
                want = fold(n, acc[y, x][None], new[y, x][None])[0]
            assert out[y, x].tobytes() == want.tobytes(), (x, y, n)
            assert nxt[y, x] == min(n + 1, 32)


def test_the_cap_holds_and_weighs_new_frames_by_one_over_cap_plus_one():
    acc, cnt = np.full((2, 2, 4), 1.0, F32), np.zeros((2, 2), np.uint32)
    for k in range(12):
        acc, cnt = H.accumulate_history(acc, cnt, np.full((2, 2, 4), float(k), F32), 4)
        assert (cnt == min(k + 1, 4)).all()
    before = acc.copy()
    acc, cnt = H.accumulate_history(acc, cnt, np.full((2, 2, 4), 100.0, F32), 4)
    assert (cnt == 4).all()
    assert np.allclose(acc[..., :3], (100.0 + before[..., :3] * 4) / 5) and (acc[..., 3] == 1.0).all()


@pytest.mark.parametrize("dtype", [np.uint8, F32])
@pytest.mark.parametrize("name", ["box", "spheres"])
def test_identity_view_with_nearest_returns_the_history_unchanged(name, dtype):
    (vp, _), (hp, _), *_ = oracle_move(name)
    rng = np.random.default_rng(11)
    h, w = hp.shape
    acc = random_image(rng, h, w, dtype)
    cnt = rng.integers(0, 3, (h, w)).astype(np.uint32) * 7
    if dtype == F32:
        acc[3, 4] = (np.nan, np.inf, -0.0, 0.25)
        cnt[3, 4] = 9
    out, ncnt = H.reproject(acc, cnt, vp, hp, vp, hp, H.NEAREST)
    u, wv, ok, _, _ = H.source_coords(vp, vp, hp)
    ys, xs = np.mgrid[0:h, 0:w]
    assert ok.all() and np.abs(u - xs).max() < 1e-4 and np.abs(wv - ys).max() < 1e-4
    assert np.array_equal(ncnt, cnt)
    held = cnt > 0
    assert held.any() and (~held).any()
    assert out[held].tobytes() == acc[held].tobytes()  # bit for bit, alpha included
    cleared = np.array([0, 0, 0, 255], np.uint8) if dtype == np.uint8 else np.array([0, 0, 0, 1], F32)
    assert (out[~held] == cleared).all()


@pytest.mark.parametrize("filt", [H.NEAREST, H.BILINEAR])
@pytest.mark.parametrize("name", ["box", "spheres"])
def test_a_rejected_pixel_has_count_zero_and_a_cleared_texel(name, filt):
    (vp, vc), (hp, hc), old, _, _ = oracle_move(name)
    acc, cnt = history_of(old[:3])
    acc[..., :3] += F32(0.5)  # no texel of the history is (0, 0, 0)
    out, ncnt = H.reproject(acc, cnt, vp, hp, vc, hc, filt)
    rejected = ncnt == 0
    assert rejected.any() and (~rejected).any() and (ncnt[~rejected] == 3).all()
    assert (out[rejected] == np.array([0, 0, 0, 1], F32)).all()
    assert (out[~rejected][:, :3] > 0).all() and (out[..., 3] == 1.0).all()
    # behind the previous camera: the view turned right round rejects everything
    back = copy.deepcopy(vc)
    m = np.array(vc.cam_alignment_mat, F32)
    m[0:3] = -m[0:3]
    back.cam_alignment_mat[:] = [float(v) for v in m]
    sky = make_hits(*hc.shape)
    _, n2 = H.reproject(acc, cnt, vp, sky, back, sky, filt)
    assert (n2 == 0).all()


@pytest.mark.parametrize("shift", [1, 5, -3])
def test_a_sideways_pan_by_whole_pixels_shifts_a_sky_only_view_by_that_many_pixels(shift):
    """Sky is reprojected by direction alone.  The pan: the same camera with the grid of ray centres moved by
    `shift` whole pixel steps (grid_first differs by shift * grid_dx), so that the direction of pixel (x, y) of
    the new view is that of pixel (x + shift, y) of the old one."""
    cam, settings = E.preset("spheres")
    h, w = 23, 37
    vp = E.View(cam, (w, h), settings).record
    vc = copy.deepcopy(vp)
    for k in range(3):
        vc.grid_first[k] = float(F32(vp.grid_first[k]) + F32(vp.grid_dx[k]) * F32(shift))
    sky = make_hits(h, w)
    rng = np.random.default_rng(2)
    acc, cnt = random_image(rng, h, w, F32), rng.integers(1, 40, (h, w)).astype(np.uint32)
    out, ncnt = H.reproject(acc, cnt, vp, sky, vc, sky, H.NEAREST)
    xs = np.arange(w)
    inside = (xs + shift >= 0) & (xs + shift < w)
    src = np.clip(xs + shift, 0, w - 1)
    assert np.array_equal(ncnt[:, inside], cnt[:, src[inside]]) and (ncnt[:, ~inside] == 0).all()
    assert out[:, inside].tobytes() == acc[:, src[inside]].tobytes()
    # the bilinear filter at whole-pixel coordinates is the same shift up to the rounding of u and w
    outb, ncntb = H.reproject(acc, cnt, vp, sky, vc, sky, H.BILINEAR)
    core = inside & (xs + shift >= 1) & (xs + shift < w - 1)
    assert np.abs(outb[1:-1, core, :3] - acc[1:-1, src[core], :3]).max() < 1e-3
    assert (ncntb[1:-1, core] > 0).all()


def test_a_tap_on_another_surface_or_at_another_depth_is_dropped():
    cam, settings = E.preset("box")
    h, w = 8, 8
    v = E.View(cam, (w, h), settings).record
    wall = make_hits(h, w, kind=2, mesh=0, index=3, t=2.0, normal=(1.0, 0.0, 0.0))
    acc, cnt = np.full((h, w, 4), 0.5, F32), np.full((h, w), 4, np.uint32)
    # a block of the previous view's records differs; u and w equal x and y up to rounding, so a bilinear tap of
    # weight ~1e-6 may reach one pixel further: the block's interior loses its history, everything outside keeps it
    block = np.zeros((h, w), bool)
    block[1:6, 2:5] = True
    for change in ({"mesh": 1}, {"t": 2.1}, {"normal": (0.0, 1.0, 0.0)}, {"kind": 0}):
        prev = wall.copy()
        for f, val in change.items():
            prev[f][block] = val
        for filt in (H.NEAREST, H.BILINEAR):
            _, n = H.reproject(acc, cnt, v, prev, v, wall, filt)
            assert (n[2:5, 3] == 0).all() and (n[~block] == 4).all(), (change, filt)
            if filt == H.NEAREST:
                assert (n[block] == 0).all()
    # tolerance 0.1 and min_normal_dot -2 accept the depth and the normal again
    prev = wall.copy()
    prev["t"][block], prev["normal"][block] = 2.1, (0.0, 1.0, 0.0)
    assert (H.reproject(acc, cnt, v, prev, v, wall, H.NEAREST, 0.1, -2.0)[1] == 4).all()


@pytest.mark.parametrize("filt", [H.NEAREST, H.BILINEAR])
@pytest.mark.parametrize("name", ["box", "spheres"])
def test_reprojected_history_beats_a_restart_after_the_move(name, filt):
    (vp, vc), (hp, hc), old, new, target = oracle_move(name)
    assert H.DEFAULTS == _lib.REPROJECT_DEFAULTS
    tgt = target[..., :3].astype(np.float64)

    def mse(a):
        return float(((a[..., :3] - tgt) ** 2).mean())

    acc, cnt = history_of(old)
    assert (cnt == 16).all()
    acc, cnt = H.reproject(acc, cnt, vp, hp, vc, hc, filt, *H.DEFAULTS)
    kept = float((cnt > 0).mean())
    assert 0.5 < kept < 1.0
    racc, rcnt = np.zeros_like(acc), np.zeros_like(cnt)
    for k, frame in enumerate(new, 1):
        acc, cnt = H.accumulate_history(acc, cnt, frame, 32)
        racc, rcnt = H.accumulate_history(racc, rcnt, frame, 32)
        if k in (1, 2, 4):
            print(f"{name} filter {filt} kept {kept:.3f} k={k}: mse reprojected {mse(acc):.6f}, restarted {mse(racc):.6f}")
            assert mse(acc) < mse(racc)
    assert same_floats(acc[..., 3], np.ones(SIZE[::-1], F32)).all()
