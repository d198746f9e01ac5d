"""Temporal upsampling on the device (hrt_set_ray_grid / hrt_accumulate_history_from): the
accumulator, the count image and the moments image byte for byte against the numpy restatement of S20
(tests/resolve_ref.py), NaN compared as NaN -- every size, both modes, every flag combination, unguided and guided
by the two contexts' real first hits, from uniform counts around max_history and from the non-uniform counts a chain
of phases leaves.  Then source == ctx against hrt_accumulate_history[_moments], the ordering without host waits,
hrt_set_ray_grid against uploaded rays, what the calls leave alone, the rejections, and the Python and C++ mirrors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import resolve_ref as R
from helpers import E, SceneCase, _lib
from image_ref import same_floats
from test_gpu_denoise import DevBuf, equal, report, synthetic_source

pytestmark = pytest.mark.gpu

F32 = np.float32
TRACE, ACCUM = _lib.IMG_TRACE, _lib.IMG_ACCUM
RGBA8, RGBA32F = _lib.FMT_RGBA8, _lib.FMT_RGBA32F
MODES = [_lib.MODE_RGBA8, _lib.MODE_RGBA32F]
FILL, MOMENTS = _lib.RESOLVE_FILL, _lib.RESOLVE_MOMENTS
# (ws, hs, w, h): source -> target
SIZES = [(1, 1, 1, 1), (1, 1, 3, 2), (5, 3, 10, 6), (5, 3, 13, 7), (37, 23, 74, 46), (37, 23, 100, 50), (64, 36, 128, 72),
         (16, 16, 8, 8)]
MAX_HISTORY = 8
COUNTS = [0, 3, MAX_HISTORY, MAX_HISTORY + 1, 1 << 24]  # none, below, at and above max_history, the largest


def native(mode):
    return RGBA8 if mode == _lib.MODE_RGBA8 else RGBA32F


def grid_of(case):
    s = case.settings
    return E.ray_grid(case.size, s.camera_focal_length, s.viewport_height, s.up)[:3]


def grid_rays(case, offset=(0.0, 0.0)):
    """The ray records of case's grid shifted by offset pixels: (first' + dx * x) + dy * y in binary32."""
    first, dx, dy = grid_of(case)
    first = E.shifted_first(first, dx, dy, *offset)
    w, h = case.size
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs.astype(F32)[..., None], ys.astype(F32)[..., None]
    c = ((first + dx * fx).astype(F32) + (dy * fy).astype(F32)).astype(F32)
    rays = np.zeros(w * h, dtype=_lib.RAY_DTYPE)
    rays["sample_centre"][:, :3] = c.reshape(-1, 3)
    rays["sample_centre"][:, 3] = 1.0
    return rays


def state(ctx, mode):
    return ctx.read(ACCUM, native(mode)), ctx.read_history(), ctx.read_moments()


def check_state(ctx, mode, want, what):
    acc, cnt, mom = state(ctx, mode)
    assert equal(acc, want[0]), (what, "A", report(acc, want[0]))
    assert np.array_equal(cnt, want[1]), (what, "N", np.argwhere(cnt != want[1])[:3])
    assert same_floats(mom, want[2]).all(), (what, "M", np.argwhere(~same_floats(mom, want[2]).all(-1))[:3])


def pair(name, size, mode, debug=True, source_options=None):
    ws, hs, w, h = size
    sc = SceneCase(name, (ws, hs), num_samples=1, max_bounces=2)
    tc = SceneCase(name, (w, h), num_samples=1, max_bounces=2)
    return sc, tc, sc.context(mode=mode, debug=debug, options=source_options), tc.context(mode=mode, debug=debug)


# ---- 1. every byte against the restatement -----------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_bytes_against_the_restatement(size, mode):
    ws, hs, w, h = size
    name = "spheres" if w == 100 else "box"
    sc, tc, src, tgt = pair(name, size, mode)
    grid = grid_of(sc)
    nx, ny = R.phases(ws, w), R.phases(hs, h)
    d_lo, d_hi = DevBuf(ws * hs * 32), DevBuf(w * h * 32)
    src.first_hits(sc.push(), d_lo.ptr)
    tgt.first_hits(tc.push(), d_hi.ptr)
    src.synchronize()
    tgt.synchronize()
    lo = d_lo.read().view(_lib.HIT_DTYPE).reshape(hs, ws)
    hi = d_hi.read().view(_lib.HIT_DTYPE).reshape(h, w)
    loaded = synthetic_source(w, h, mode)  # float mode: NaN and infinite texels among them
    accepted_any = filled_any = rejected_by_guide = False
    shot = 0
    for count in COUNTS:
        for flags in (0, FILL, MOMENTS, FILL | MOMENTS):
            for guided in (False, True):
                k = shot % (nx * ny)
                shot += 1
                off = R.history_phase(ws, w, hs, h, k)
                src.shift_ray_grid(off[0], off[1], grid)
                src.trace(sc.push(1 + shot))
                tex = src.read(TRACE, native(mode))
                tgt.load_accumulator(loaded)
                tgt.fill_history(count)
                tgt.fill_moments(0.3, 0.2)
                acc0, cnt0, mom0 = state(tgt, mode)
                assert (cnt0 == count).all()
                info = tgt.resolve_info(off, MAX_HISTORY)
                info.flags = flags
                tgt.accumulate_history_from(src, info=info, source_hits_ptr=d_lo.ptr if guided else None,
                                            hits_ptr=d_hi.ptr if guided else None)
                want = R.resolve(acc0, cnt0, mom0, tex, off, MAX_HISTORY, flags, lo if guided else None, hi if guided else None)
                check_state(tgt, mode, want[:3], (size, count, flags, guided, k))
                plain = R.resolve(acc0, cnt0, mom0, tex, off, MAX_HISTORY, flags)[3]
                accepted_any |= bool(want[3].any())
                filled_any |= bool(want[4].any())
                rejected_by_guide |= guided and bool((plain & ~want[3]).any())
                # the source's trace image and the guides are only read
                assert src.read(TRACE, native(mode)).tobytes() == tex.tobytes()
    assert accepted_any and (filled_any or nx * ny == 1)
    if min(ws, hs) >= 16 and nx * ny > 1:
        assert rejected_by_guide  # (a silhouette pixel whose low sample shows the other surface)
    # a chain of nx * ny + 1 phases from an empty history: non-uniform counts, every pixel sampled
    tgt.load_accumulator(loaded)
    tgt.fill_history(0)
    tgt.fill_moments(0.0, 0.0)
    want = state(tgt, mode)
    for k in range(nx * ny + 1):
        off = R.history_phase(ws, w, hs, h, k)
        src.shift_ray_grid(off[0], off[1], grid)
        src.trace(sc.push(100 + k))
        tex = src.read(TRACE, native(mode))
        tgt.accumulate_history_from(src, off, 3, moments=True, fill=True)
        want = R.resolve(want[0], want[1], want[2], tex, off, 3, FILL | MOMENTS)[:3]
        check_state(tgt, mode, want, (size, "chain", k))
    assert (want[1] >= 1).all() and (nx * ny == 1 or len(np.unique(want[1])) > 1)
    assert d_lo.read().tobytes() == lo.tobytes() and d_hi.read().tobytes() == hi.tobytes()
    for c in (src, tgt):
        n, bad = c.check_guards()
        assert n > 0 and bad == 0
        c.close()
    d_lo.free()
    d_hi.free()


@pytest.mark.parametrize("mode", MODES)
def test_synthetic_guides_that_disagree_on_a_block(mode):
    size = ws, hs, w, h = 37, 23, 74, 46
    sc, tc, src, tgt = pair("box", size, mode)
    src.trace(sc.push(3))
    tex = src.read(TRACE, native(mode))
    lo, hi = np.zeros((hs, ws), _lib.HIT_DTYPE), np.zeros((h, w), _lib.HIT_DTYPE)
    lo["kind"], lo["index"], lo["mesh"] = 2, 5, 1
    hi["kind"], hi["index"], hi["mesh"] = 2, 9, 1       # another triangle of the same mesh: the same key
    hi["mesh"][10:30, 20:50] = 2                         # a block of another mesh
    hi["kind"][0:4, 0:6] = 0                             # and a corner of misses
    d_lo, d_hi = DevBuf(lo.nbytes).write(lo), DevBuf(hi.nbytes).write(hi)
    tgt.fill_history(2)
    tgt.fill_moments(0.5, 0.5)
    tgt.load_accumulator(synthetic_source(w, h, mode))
    before = state(tgt, mode)
    off = R.history_phase(ws, w, hs, h, 0)
    tgt.accumulate_history_from(src, off, MAX_HISTORY, moments=True, source_hits_ptr=d_lo.ptr, hits_ptr=d_hi.ptr)
    want = R.resolve(*before, tex, off, MAX_HISTORY, FILL | MOMENTS, lo, hi)
    check_state(tgt, mode, want[:3], "block")
    plain = R.resolve(*before, tex, off, MAX_HISTORY, FILL | MOMENTS)[3]
    same_key = D.surface_keys(hi) == D.surface_keys(lo)[0, 0]
    assert np.array_equal(want[3], plain & same_key) and 0 < want[3].sum() < plain.sum()
    src.close()
    tgt.close()
    d_lo.free()
    d_hi.free()


# ---- 2. source == ctx is hrt_accumulate_history ---------------------------------------------------------------------

@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_the_same_context_gives_accumulate_history(mode, moments):
    size = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode), case.context(mode=mode)
    for frame in range(5):  # counts pass max_history = 3 on the way
        for c in (ctx, twin):
            c.trace(case.push(1 + frame))
        ctx.accumulate_history_from(ctx, (0.0, 0.0), 3, moments=moments, fill=False)
        if moments:
            twin.accumulate_history_moments(3)
        else:
            twin.accumulate_history(3)
        a, b = state(ctx, mode), state(twin, mode)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), frame
        assert ctx.stats().accumulates == twin.stats().accumulates
    ctx.close()
    twin.close()


# ---- 3. ordering: no host wait between the calls ---------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_unsynchronised_calls_give_the_synchronised_chain(mode, deferred, lanes):
    """Eight frames of (set_ray_grid, trace on the source, fold on the target) with no synchronisation give the bytes
    of the chain synchronised after every call.  The target's stream is kept busy ahead of every fold (a many-sample frame
    of its own and a first-hit pass), so that the fold lags the source: with one trace lane (lanes = 1) the
    source's very next trace writes the image the queued fold still has to read, and only the device-side wait
    holds it back -- also across the hrt_set_ray_grid, hrt_accumulate and trace-image read that the source issues in
    between, each of which re-records the lane's own events."""
    size = ws, hs, w, h = 120, 68, 240, 136
    opts = {_lib.OPT_DEFER_COMBINE: 1} if deferred else {}
    if lanes:
        opts[_lib.OPT_OVERLAP] = lanes
    results = []
    for synced in (False, True):
        sc, tc, src, tgt = pair("spheres", size, mode, debug=False, source_options=opts)
        grid = grid_of(sc)
        d_hi = DevBuf(w * h * 32)
        for k in range(8):
            off = R.history_phase(ws, w, hs, h, k)
            src.shift_ray_grid(off[0], off[1], grid)
            if synced:
                src.synchronize()
            src.trace(sc.push(1 + k))
            if synced:
                src.synchronize()
            if deferred:
                src.accumulate(k)  # (recorded, folded later: the source has deferred combines when the fold runs)
            # work queued on the target's stream ahead of the fold, far longer than the source's next 1-sample trace:
            # a 32-sample frame of the target's own (hrt_compute_n runs on the context's stream) and its first hits
            heavy = tc.push(50 + k)
            heavy.num_samples, heavy.max_bounces = 32, 4
            tgt.compute_n(heavy, 1)
            tgt.first_hits(tc.push(), d_hi.ptr)
            tgt.accumulate_history_from(src, off, MAX_HISTORY, moments=True)
            if not deferred and k == 3 and not synced:
                src.accumulate(k)  # a source-side call that re-records the lane's own event, right behind the fold
            if synced:
                src.synchronize()
                tgt.synchronize()
                if not deferred and k == 3:
                    src.accumulate(k)
        results.append([a.tobytes() for a in state(tgt, mode)] + [src.read(ACCUM, native(mode)).tobytes(),
                                                                 src.read(TRACE, native(mode)).tobytes()])
        src.close()
        tgt.close()
        d_hi.free()
    assert results[0] == results[1]


# ---- 4. hrt_set_ray_grid ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_set_ray_grid_against_uploaded_rays(mode):
    size = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    first, dx, dy = grid_of(case)
    ctx = case.context(mode=mode)
    # the unshifted grid is the host's rays bit for bit
    ctx.set_ray_grid(first, dx, dy)
    assert ctx.read_rays().tobytes() == case.rays[:case.n_rays].tobytes()
    assert grid_rays(case).tobytes() == case.rays[:case.n_rays].tobytes()
    ctx.trace(case.push(1))  # a trace with these rays: tile lists that the next grid makes stale
    before = ctx.read(TRACE, native(mode))
    off = (0.25, -0.5)
    rays = grid_rays(case, off)
    twin = E.HrtContext(size, device=0, mode=mode)
    twin.set_scene(rays, case.spheres, case.tris, case.meshes)
    ctx.shift_ray_grid(off[0], off[1])  # (the base grid is the last set_ray_grid's)
    assert ctx.read_rays().tobytes() == rays.tobytes() == twin.read_rays().tobytes()
    d_a, d_b = DevBuf(size[0] * size[1] * 32), DevBuf(size[0] * size[1] * 32)
    for frame in (1, 2):
        for c in (ctx, twin):
            c.trace(case.push(frame))
        got, want = ctx.read(TRACE, native(mode)), twin.read(TRACE, native(mode))
        assert got.tobytes() == want.tobytes(), frame
    assert got.tobytes() != before.tobytes()  # (other rays, another frame)
    for method in (_lib.FIRST_HITS_TILES, _lib.FIRST_HITS_QUERY):
        ctx.first_hits(case.push(), d_a.ptr, method)
        twin.first_hits(case.push(), d_b.ptr, method)
        ctx.synchronize()
        twin.synchronize()
        assert d_a.read().tobytes() == d_b.read().tobytes(), method
    assert ctx.intersect_primary(case.push()).tobytes() == twin.intersect_primary(case.push()).tobytes()
    # a later hrt_set_scene(rays = NULL) keeps the new rays
    ctx.set_scene(None, case.spheres, case.tris, case.meshes)
    assert ctx.read_rays().tobytes() == rays.tobytes()
    ctx.trace(case.push(2))
    assert ctx.read(TRACE, native(mode)).tobytes() == twin.read(TRACE, native(mode)).tobytes()
    # set, trace, set, trace with nothing in between: each trace sees its own grid
    ctx.set_ray_grid(first, dx, dy)
    ctx.trace(case.push(1))
    ctx.shift_ray_grid(off[0], off[1])
    ctx.trace(case.push(1))
    ctx.set_ray_grid(first, dx, dy)
    twin.trace(case.push(1))
    assert ctx.read(TRACE, native(mode)).tobytes() == twin.read(TRACE, native(mode)).tobytes()
    assert ctx.read_rays().tobytes() == case.rays[:case.n_rays].tobytes()
    # a context that never had rays gets its buffer from the call
    bare = E.HrtContext(size, device=0, mode=mode)
    bare.shift_ray_grid(off[0], off[1], (first, dx, dy))
    bare.set_scene(None, case.spheres, case.tris, case.meshes)
    bare.trace(case.push(1))
    twin.trace(case.push(1))
    assert bare.read(TRACE, native(mode)).tobytes() == twin.read(TRACE, native(mode)).tobytes()
    for c in (ctx, twin, bare):
        c.close()
    d_a.free()
    d_b.free()


# ---- 5. what the calls leave alone, and the rejections ---------------------------------------------------------------

def _stats_tuple(st):
    # (timings and wave_steps depend on scheduling: tests/test_gpu_intersect.py)
    return (st.segments, st.tri_tests, st.traces, st.accumulates, st.last_kernel, st.last_block, st.last_frames)


@pytest.mark.parametrize("mode", MODES)
def test_the_call_leaves_the_rest_alone(mode):
    size = ws, hs, w, h = 37, 23, 74, 46
    sc, tc, src, tgt = pair("box", size, mode)
    for frame in range(2):
        src.trace(sc.push(1 + frame))
        src.accumulate_history_moments(4)
    src.trace(sc.push(7))
    tgt.trace(tc.push(3))
    before_src = (src.read(TRACE, native(mode)), *state(src, mode), _stats_tuple(src.stats()))
    before_tgt = (tgt.read(TRACE, native(mode)), _stats_tuple(tgt.stats()))
    for k in range(5):
        off = R.history_phase(ws, w, hs, h, k)
        tgt.accumulate_history_from(src, off, MAX_HISTORY, moments=bool(k & 1))
    after_src = (src.read(TRACE, native(mode)), *state(src, mode), _stats_tuple(src.stats()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before_src[:4], after_src[:4])) and before_src[4] == after_src[4]
    st = _stats_tuple(tgt.stats())
    assert tgt.read(TRACE, native(mode)).tobytes() == before_tgt[0].tobytes()
    assert st[:3] == before_tgt[1][:3] and st[3] == before_tgt[1][3] + 5 and st[4:] == before_tgt[1][4:]
    for c in (src, tgt):
        assert c.check_guards()[1] == 0
        c.close()


def test_rejections_enqueue_nothing_and_leave_both_contexts_usable():
    size = ws, hs, w, h = 37, 23, 74, 46
    mode = _lib.MODE_RGBA32F
    sc, tc, src, tgt = pair("box", size, mode, debug=False)
    src.trace(sc.push(1))
    tgt.accumulate_history_from(src, (0.25, 0.25), MAX_HISTORY, moments=True)
    before = [a.tobytes() for a in state(tgt, mode)]
    rays_before = src.read_rays().tobytes()
    lib, handle = tgt.lib, tgt.handle
    d_lo, d_hi = DevBuf(ws * hs * 32 + 16), DevBuf(w * h * 32 + 16)
    host_hits = np.zeros(w * h, dtype=_lib.HIT_DTYPE)
    good = tgt.resolve_info((0.25, 0.25), MAX_HISTORY, moments=True)

    def raw(ctx=handle, source=src.handle, info=good, lo=d_lo.ptr, hi=d_hi.ptr):
        return lib.hrt_accumulate_history_from(ctx, source, ctypes.byref(info) if info is not None else None,
                                               ctypes.c_void_p(lo or 0), ctypes.c_void_p(hi or 0))

    def altered(**kw):
        info = tgt.resolve_info((0.25, 0.25), MAX_HISTORY, moments=True)
        for k, v in kw.items():
            setattr(info, k, v)
        return info

    assert raw(ctx=None) == 1
    assert raw(source=None) == 1 and b"null source" in lib.hrt_last_error(handle)
    assert raw(info=None) == 1 and b"null info" in lib.hrt_last_error(handle)
    for field in ("offset_x", "offset_y"):
        for v in (float("nan"), float("inf"), -float("inf"), 0.5000001, -0.75, 3.0):
            assert raw(info=altered(**{field: v})) == 1 and b"offsets" in lib.hrt_last_error(handle), (field, v)
    for v in (0, (1 << 24) + 1, 0xFFFFFFFF):
        assert raw(info=altered(max_history=v)) == 1 and b"max_history" in lib.hrt_last_error(handle), v
    for v in (4, 8, 0x80000000, 7):
        assert raw(info=altered(flags=v)) == 1 and b"flag" in lib.hrt_last_error(handle), v
    assert raw(lo=None) == 1 and b"both" in lib.hrt_last_error(handle)
    assert raw(hi=None) == 1 and b"both" in lib.hrt_last_error(handle)
    assert raw(lo=d_lo.ptr + 8) == 1 and b"aligned" in lib.hrt_last_error(handle)
    assert raw(hi=d_hi.ptr + 8) == 1 and b"aligned" in lib.hrt_last_error(handle)
    assert raw(lo=host_hits.ctypes.data) == 1 and b"source_hits" in lib.hrt_last_error(handle)
    assert raw(hi=host_hits.ctypes.data) == 1 and b"hits" in lib.hrt_last_error(handle)
    other_mode = sc.context(mode=_lib.MODE_RGBA8)
    assert raw(source=other_mode.handle, lo=None, hi=None) == 1 and b"modes" in lib.hrt_last_error(handle)
    other_mode.close()
    no_scene = E.HrtContext((ws, hs), device=0, mode=mode)
    assert raw(source=no_scene.handle, lo=None, hi=None) == 4 and b"scene" in lib.hrt_last_error(handle)  # HRT_ERR_NO_SCENE
    no_scene.close()
    # hrt_set_ray_grid
    v, nan, inf = _lib.f3((1.0, 0.5, 0.25)), _lib.f3((1.0, float("nan"), 0.0)), _lib.f3((float("inf"), 0.0, 0.0))
    sh = src.handle
    assert lib.hrt_set_ray_grid(sh, None, v, v) == 1 and lib.hrt_set_ray_grid(sh, v, None, v) == 1
    assert lib.hrt_set_ray_grid(sh, v, v, None) == 1 and b"null" in lib.hrt_last_error(sh)
    for bad in (nan, inf):
        for args in ((bad, v, v), (v, bad, v), (v, v, bad)):
            assert lib.hrt_set_ray_grid(sh, *args) == 1 and b"finite" in lib.hrt_last_error(sh)
    # nothing was enqueued: the state, the rays and the next results are those of a pair that saw no rejection
    assert [a.tobytes() for a in state(tgt, mode)] == before and src.read_rays().tobytes() == rays_before
    sc2, tc2, src2, tgt2 = pair("box", size, mode, debug=False)
    for s, t, case in ((src, tgt, sc), (src2, tgt2, sc2)):
        if s is src2:
            s.trace(case.push(1))
            t.accumulate_history_from(s, (0.25, 0.25), MAX_HISTORY, moments=True)
        s.trace(case.push(2))
        t.accumulate_history_from(s, (-0.25, 0.25), MAX_HISTORY, moments=True)
    assert [a.tobytes() for a in state(tgt, mode)] == [a.tobytes() for a in state(tgt2, mode)]
    for c in (src, tgt, src2, tgt2):
        c.close()
    # a row-tile partition, with and without a communicator, and an unpartitioned context joined to one
    whole = sc.context(mode=mode)
    parts = [sc.context(mode=mode, partition=(8, p, 2)) for p in range(2)]
    g = grid_of(sc)
    for joined in (False, True):
        if joined:
            E.HrtContext.comm_init_all(parts)
        for c in parts:
            with pytest.raises(_lib.HrtError, match="partition"):
                c.accumulate_history_from(whole)
            with pytest.raises(_lib.HrtError, match="partition"):
                whole.accumulate_history_from(c)
            with pytest.raises(_lib.HrtError, match="partition"):
                c.set_ray_grid(*g)
    for c in parts:
        c.close()
    single = sc.context(mode=mode)
    E.HrtContext.comm_init_all([single])
    with pytest.raises(_lib.HrtError, match="communicator"):
        single.accumulate_history_from(whole)
    with pytest.raises(_lib.HrtError, match="communicator"):
        whole.accumulate_history_from(single)
    with pytest.raises(_lib.HrtError, match="communicator"):
        single.set_ray_grid(*g)
    single.close()
    whole.close()
    d_lo.free()
    d_hi.free()


def test_another_device_is_rejected():
    n = ctypes.c_int(0)
    assert ctypes.CDLL("libamdhip64.so").hipGetDeviceCount(ctypes.byref(n)) == 0
    if n.value < 2:
        pytest.skip("one device: a pair on different devices cannot be made")
    a, b = E.HrtContext((8, 8), device=0), E.HrtContext((8, 8), device=1)
    with pytest.raises(_lib.HrtError, match="different devices"):
        a.accumulate_history_from(b)
    a.close()
    b.close()


# ---- 6. the mirrors --------------------------------------------------------------------------------------------------

def demo_settings():
    """upsample_demo's / resolve_demo's scene through the Python mirror: the box scene's geometry, Lambertian grey,
    1 sample, 4 bounces, light on."""
    _, settings = E.preset("box")
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    return settings, E.RayTracerSettings(num_samples=1, max_bounces=4, use_environment_lighting=True,
                                         sphere_data=[E.Sphere(s.centre, s.radius, grey) for s in settings.sphere_data],
                                         mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in settings.mesh_data])


def python_mirror_chain(st, frames=5):
    """RayTracePipeline.shift_rays + DiffusePipeline.next_frame_history_from: (A, N, M) of the 48 x 32 history and the
    per-frame trace images and offsets."""
    (ws, hs), (w, h) = (24, 16), (48, 32)
    low, high = E.HrtContext((ws, hs), device=0, mode=_lib.MODE_RGBA32F), E.HrtContext((w, h), device=0, mode=_lib.MODE_RGBA32F)
    pipe, diffuse, cam = E.RayTracePipeline(low, (ws, hs), st), E.DiffusePipeline(high, (w, h)), E.Camera()
    steps = []
    for frame in range(frames):
        off = E.history_phase((ws, hs), (w, h), frame)
        pipe.shift_rays(*off)
        pipe.compute(cam, frame)
        diffuse.next_frame_history_from(pipe.image(), off, moments=True)
        steps.append((off, low.read(TRACE, RGBA32F)))
    out = state(high, _lib.MODE_RGBA32F)
    pipe.shift_rays(0.0, 0.0)
    assert low.read_rays().tobytes() == pipe.rays.tobytes()  # (0, 0) restores the pipeline's own rays
    # a View of a shifted grid is the view of those rays
    v = E.View(cam, (ws, hs), st, offset=(0.25, -0.25)).record
    pipe.shift_rays(0.25, -0.25)
    assert np.array_equal(low.read_rays()["sample_centre"][0, :3], np.array(v.grid_first[:3], F32))
    low.close()
    high.close()
    return out, steps


def test_pipeline_mirror():
    _, st = demo_settings()
    (acc, cnt, mom), steps = python_mirror_chain(st)
    (ws, hs), (w, h) = (24, 16), (48, 32)
    want = (np.zeros((h, w, 4), F32), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32))
    want[0][..., 3] = 1.0  # (a new context's accumulator is cleared)
    for k, (off, tex) in enumerate(steps):
        assert off == tuple(float(v) for v in R.history_phase(ws, w, hs, h, k))
        want = R.resolve(*want, tex, off, R.DEFAULT_MAX_HISTORY, FILL | MOMENTS)[:3]
    assert equal(acc, want[0]) and np.array_equal(cnt, want[1]) and same_floats(mom, want[2]).all()
    assert cnt.min() == 1 and cnt.max() == 2  # four phases cover the image, the fifth revisits the first's pixels


def test_cpp_mirror_resolve(tmp_path):
    """include/hrt_app.hpp's set_ray_grid / history_phase / accumulate_history_from (tests/cpp/resolve_demo) give the
    Python mirror's bytes on the box scene's geometry."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "resolve_demo.mk", "resolve_demo"], check=True)  # (up to date after build())
    settings, st = demo_settings()
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        f.write(np.uint32(len(settings.sphere_data)).tobytes())
        for s in settings.sphere_data:
            f.write(np.float32([*s.centre, s.radius]).tobytes())
        f.write(np.uint32(len(settings.mesh_data)).tobytes())
        for m in settings.mesh_data:
            f.write(np.uint32([len(m.mesh.positions), len(m.mesh.indices)]).tobytes())
            f.write(m.mesh.positions.tobytes())
            f.write(m.mesh.indices.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([os.path.join(cpp, "resolve_demo"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    w, h = 48, 32
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [w, h] and len(raw) == 8 + w * h * (16 + 4 + 8)
    (acc, cnt, mom), _ = python_mirror_chain(st)
    assert raw[8:8 + w * h * 16] == acc.tobytes()
    assert raw[8 + w * h * 16:8 + w * h * 20] == cnt.tobytes()
    assert raw[8 + w * h * 20:] == mom.tobytes()
