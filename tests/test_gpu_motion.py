"""Object motion in the temporal history on the device (hrt_reproject_motion, hrt_reproject_motion_moments; DESIGN.md
§2 S21, §36): every byte of the accumulator, the count image and the moments image against the numpy restatement of
S21 (tests/motion_ref.py), NaN compared as NaN, in both context modes and both filters.  Guides are synthetic (several
objects per wave and tile, tables that mix moving, static, out-of-range and NULL entries) or the real first hits of
spheres and box before and after a real move of one object (hrt_set_scene twice, motion_between for the table).  Then
the static twin, the lifetime of the caller's tables, the rejections, what the calls leave alone, and the mirrors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import history_ref as H
import motion_ref as M
import present_ref
import variance_ref as V
from helpers import E, SceneCase, _lib
from test_gpu_history import CAP, DevBuf, synthetic_guide, synthetic_source, view_pairs
from test_gpu_variance import check_state, equal, native, report, traced_moments

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xA5
TRACE, ACCUM = _lib.IMG_TRACE, _lib.IMG_ACCUM
RGBA8, RGBA32F = _lib.FMT_RGBA8, _lib.FMT_RGBA32F
MODES = [_lib.MODE_RGBA8, _lib.MODE_RGBA32F]
FILTERS = [_lib.REPROJECT_NEAREST, _lib.REPROJECT_BILINEAR]
SIZES = [(1, 1), (2, 2), (37, 23), (64, 64), (130, 70)]  # (width, height)
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def pose(r=None, t=(0, 0, 0)):
    """A column-major 3x4 [R | t] as 12 float32."""
    r = np.eye(3) if r is None else r
    return np.concatenate([np.asarray(r, np.float64).T.reshape(9), np.asarray(t, np.float64)]).astype(F32)


def tables_arg(spheres, meshes):
    """_lib.MotionTables over two motion_ref.MOTION arrays (None: NULL, count 0)."""
    return _lib.MotionTables(spheres.ctypes.data if spheres is not None and len(spheres) else None,
                             len(spheres) if spheres is not None else 0,
                             meshes.ctypes.data if meshes is not None and len(meshes) else None,
                             len(meshes) if meshes is not None else 0)


def call(ctx, prev, d_prev, cur, d_cur, spheres, meshes, moments, **fields):
    ctx.reproject_motion(prev, d_prev, cur, d_cur, moments=moments, tables=tables_arg(spheres, meshes), **fields)


def synthetic_tables(px, seed):
    """Table variants for synthetic_guide's objects (sphere indices 3..8, mesh indices 0..1): motions of a few pixels.
    px: one pixel's size at unit depth."""
    rng = np.random.default_rng(seed)

    def moving(scale=1.0):
        r = rotation(rng.normal(size=3), rng.uniform(-0.03, 0.03) * scale)
        return pose(r, rng.uniform(-12, 12, 3) * px * scale), M.MOVING

    still = (IDENTITY, 0)
    junk = (np.full(12, np.nan, F32), 0)  # a static entry's matrix is never read
    mixed_s = M.table([junk, still, still, moving(), still, moving(), moving()])  # 7, 8: out of range; 4: static
    mixed_m = M.table([moving()])                                                # mesh 1: out of range
    full = M.static(M.MAX_OBJECTS)
    full["flags"][:] = M.MOVING
    full["m"][:] = moving()[0]
    full["m"][5] = moving(2.0)[0]
    return [("mixed", mixed_s, mixed_m), ("null spheres", None, M.table([still, moving()])),
            ("cap, null meshes", full, None), ("one sphere entry", M.table([moving()]), M.table([moving(), moving()]))]


def check(ctx, mode, acc, cnt, mom, what):
    if mom is not None:
        return check_state(ctx, mode, acc, cnt, mom, what)
    got = ctx.read(ACCUM, native(mode))
    assert equal(got, acc), (what, "accumulator", report(got, acc))
    got = ctx.read_history()
    assert equal(got, cnt), (what, "counts", report(got, cnt))


# ---- 1. synthetic accumulators, counts, moments, guides and tables ----------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_motion_reprojection_of_synthetic_history(size, mode):
    w, h = size
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context(mode=mode, debug=True)
    src = synthetic_source(w, h, mode)
    prev_hits, cur_hits = synthetic_guide(w, h, seed=2), synthetic_guide(w, h, seed=2)
    rng = np.random.default_rng([7, w, h])
    change = rng.uniform(size=(h, w)) < 0.15
    prev_hits["mesh"][change & (prev_hits["kind"] == 2)] += 1
    with np.errstate(over="ignore"):
        prev_hits["t"][change & (prev_hits["kind"] == 1)] *= F32(1.01)
    d_prev, d_cur = DevBuf(w * h * 32).write(prev_hits), DevBuf(w * h * 32).write(cur_hits)
    views = view_pairs(size)[:3]  # identity, a turn, a previous camera some points lie behind
    _, _, mom0 = traced_moments(ctx, case, (3, 4))
    differs = 0
    for vi, (name, prev, cur) in enumerate(views):
        for ti, (tname, spheres, meshes) in enumerate(synthetic_tables(2.0 / h, [11, w, h])):
            for filt in FILTERS:
                moments = bool((vi + ti + filt) & 1)
                tol, mind = H.DEFAULTS if (ti & 1) else (0.5, -2.0)
                count = (CAP, 9, 1, 0, 32)[(vi + ti) % 5]  # none, one, a cap of 32 (folded with it below), 2^24
                if moments:
                    ctx.fill_history(0)
                    traced_moments(ctx, case, (3, 4))
                ctx.load_accumulator(src)
                ctx.fill_history(count)
                acc, cnt, mom = src, np.full((h, w), count, np.uint32), mom0 if moments else None
                for rep in range(2):
                    call(ctx, prev, d_prev.ptr, cur, d_cur.ptr, spheres, meshes, moments, filter=filt, depth_tolerance=tol,
                         min_normal_dot=mind)
                    args = (prev.record, prev_hits, cur.record, cur_hits, spheres, meshes, filt, tol, mind)
                    plain = H.reproject(acc, cnt, prev.record, prev_hits, cur.record, cur_hits, filt, tol, mind)
                    if moments:
                        acc, cnt, mom = M.reproject_moments(acc, cnt, mom, *args)
                    else:
                        acc, cnt = M.reproject(acc, cnt, *args)
                    check(ctx, mode, acc, cnt, mom, (name, tname, filt, moments, rep))
                    differs += int(not np.array_equal(plain[1], cnt) or not equal(plain[0], acc))
                    if rep == 0:  # mixed counts for the second pass: 0 where rejected, then one fold
                        ctx.trace(case.push(5))
                        new = ctx.read(TRACE, native(mode))
                        cap = 32 if count == 32 else CAP
                        if moments:
                            ctx.accumulate_history_moments(cap)
                            acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, cap)
                        else:
                            ctx.accumulate_history(cap)
                            acc, cnt = H.accumulate_history(acc, cnt, new, cap)
    if w * h >= 15:
        assert differs > 8  # the moving entries change the result: the cases do not pass on S15 alone
    assert d_prev.read().tobytes() == prev_hits.tobytes() and d_cur.read().tobytes() == cur_hits.tobytes()
    ctx.synchronize()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    d_prev.free()
    d_cur.free()


# ---- 2. static and empty tables: the twin's hrt_reproject[_moments], byte for byte -----------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [(37, 23), (130, 70)])
def test_static_and_empty_tables_are_the_plain_calls(size, mode):
    w, h = size
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, debug=True), case.context(mode=mode)
    src = synthetic_source(w, h, mode)
    hits = synthetic_guide(w, h)
    d_hits = DevBuf(w * h * 32).write(hits)
    _, prev, cur = view_pairs(size)[1]
    still = M.table([(np.arange(12), 0)] * 9)
    # one moving entry no pixel refers to (sphere index 0): the motion kernel itself runs, every pixel static
    unused = M.table([(pose(rotation([0, 1, 0], 0.3), [1, 2, 3]), M.MOVING)])
    for spheres, meshes in ((None, None), (still, still), (still[:0], None), (unused, still)):
        for moments in (False, True):
            for filt in FILTERS:
                for c in (ctx, twin):
                    c.fill_history(0)
                    traced_moments(c, case, (3, 4))
                    c.load_accumulator(src)
                    c.fill_history(7)
                call(ctx, prev, d_hits.ptr, cur, d_hits.ptr, spheres, meshes, moments, filter=filt)
                (twin.reproject_moments if moments else twin.reproject)(prev, d_hits.ptr, cur, d_hits.ptr, filter=filt)
                assert ctx.read(ACCUM, native(mode)).tobytes() == twin.read(ACCUM, native(mode)).tobytes()
                assert ctx.read_history().tobytes() == twin.read_history().tobytes()
                assert ctx.read_moments().tobytes() == twin.read_moments().tobytes()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    d_hits.free()


# ---- 3. real scenes: one object moved between two hrt_set_scene calls ---------------------------------------------------

def moved_settings(name, k):
    """(settings of state k, the object's pose in state k, ('sphere' | 'mesh', its index)): spheres: sphere 3 slides
    along x and y; box: the floor (mesh 0) turns about its centre in its own plane."""
    _, settings = E.preset(name)
    if name == "spheres":
        t = np.array([0.35 * k, 0.1 * k, 0.0])
        s = settings.sphere_data[3]
        settings.sphere_data[3] = E.Sphere([float(F32(c + d)) for c, d in zip(s.centre, t)], s.radius, s.material)
        return settings, pose(None, t), ("sphere", 3)
    m = settings.mesh_data[0]
    pos = np.asarray(m.mesh.positions, np.float64).reshape(-1, 3)
    centre = (pos.min(0) + pos.max(0)) / 2
    r = rotation([0, 1, 0], 0.12 * k)
    p = pose(r, centre - r @ centre)
    r32, t32 = p[:9].reshape(3, 3).T.astype(np.float64), p[9:].astype(np.float64)
    mesh = E.Mesh((pos @ r32.T + t32).astype(F32).reshape(np.asarray(m.mesh.positions).shape), m.mesh.indices)
    settings.mesh_data[0] = E.RayTracingMesh(mesh, m.material)
    return settings, p, ("mesh", 0)


def motion_tables_of(prev_pose, cur_pose, which, n_spheres, n_meshes):
    rec = E.motion_between(prev_pose, cur_pose)
    g, flags = M.motion_between(prev_pose, cur_pose)
    assert np.array(list(rec.m), F32).tobytes() == g.tobytes() and rec.flags == flags == M.MOVING
    spheres, meshes = M.static(n_spheres), M.static(n_meshes)
    tab = spheres if which[0] == "sphere" else meshes
    tab["m"][which[1]], tab["flags"][which[1]] = g, flags
    return spheres, meshes


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,size", [("spheres", (64, 64)), ("spheres", (130, 70)), ("box", (64, 64)), ("box", (130, 70))])
def test_three_frame_chain_with_a_moving_object(name, size, mode):
    w, h = size
    states = [moved_settings(name, k) for k in range(3)]
    cases = [SceneCase(name, size, num_samples=1, max_bounces=4, settings=s[0], camera=E.preset(name)[0]) for s in states]
    ctx = cases[0].context(mode=mode, debug=True)
    view = E.View(cases[0].camera, size, cases[0].settings)
    d_hits = [DevBuf(w * h * 32), DevBuf(w * h * 32)]
    acc = np.zeros((h, w, 4), np.uint8 if mode == _lib.MODE_RGBA8 else F32)
    acc[..., 3] = 255 if mode == _lib.MODE_RGBA8 else 1.0
    cnt, mom = np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    hits = None
    for k, case in enumerate(cases):
        if k:
            ctx.set_scene(case.rays, case.spheres, case.tris, case.meshes)  # keeps A, N and M
            check_state(ctx, mode, acc, cnt, mom, (k, "set_scene"))
        ctx.first_hits(case.push(), d_hits[k & 1].ptr)
        ctx.synchronize()
        cur_hits = d_hits[k & 1].read().view(_lib.HIT_DTYPE).reshape(h, w)
        if k:
            filt = FILTERS[k & 1]
            spheres, meshes = motion_tables_of(states[k - 1][1], states[k][1], states[k][2], len(case.spheres), len(case.meshes))
            call(ctx, view, d_hits[(k - 1) & 1].ptr, view, d_hits[k & 1].ptr, spheres, meshes, True, filter=filt)
            plain = H.reproject(acc, cnt, view.record, hits, view.record, cur_hits, filt, *H.DEFAULTS)
            acc, cnt, mom = M.reproject_moments(acc, cnt, mom, view.record, hits, view.record, cur_hits, spheres, meshes, filt,
                                                *H.DEFAULTS)
            check_state(ctx, mode, acc, cnt, mom, (k, "reproject"))
            # the motion matters: more than a handful of pixels differ from hrt_reproject's on the same inputs, and
            # the mover keeps history that S15 alone would drop or misregister
            other = (plain[1] != cnt) | ~(plain[0] == acc).reshape(h, w, -1).all(-1)
            assert other.sum() > 20, other.sum()
            key = M.surface_keys(cur_hits)
            mover = key == (0x80000003 if name == "spheres" else 1)
            assert mover.sum() > 20 and (cnt[mover] > 0).mean() > 0.5
        ctx.trace(case.push(1 + k))
        new = ctx.read(TRACE, native(mode))
        ctx.accumulate_history_moments(32)
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, 32)
        check_state(ctx, mode, acc, cnt, mom, (k, "fold"))
        hits = cur_hits
    # filter and present over the carried history, guided by the current first hits
    last = d_hits[(len(cases) - 1) & 1].ptr
    want, _ = V.denoise_variance(acc, cnt, mom, 3, V.DEFAULTS, hits)
    got = ctx.denoise_variance(RGBA32F, last, iterations=3)
    assert equal(got, want), report(got, want)
    target = DevBuf(w * h * 4 + 64)
    ticket = ctx.denoise_variance_present(target.ptr, w * h * 4, w, h, w * 4, _lib.PRESENT_B8G8R8A8, last, iterations=3)
    ctx.present_wait(ticket)
    want8, _ = V.denoise_variance(acc, cnt, mom, 3, V.DEFAULTS, hits, fmt_rgba8=True)
    assert target.read().tobytes() == present_ref.present_bytes(want8, w, h, w * 4, _lib.PRESENT_B8G8R8A8, target.nbytes, 0,
                                                                FILL).tobytes()
    ctx.synchronize()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    for b in d_hits + [target]:
        b.free()


# ---- 4. the caller's tables may go at once; more calls in flight than the ring is deep -------------------------------------

def lifetime_inputs(w, h, calls, seed=5):
    """A guide and a chain of tables under which history survives `calls` reprojections of the identity view pair and
    the final state depends on every call's table: four spheres in 32 x 32 blocks at one depth, each call moving every
    sphere by a pixel sideways, up or both; the tables differ in size from call to call (static padding entries
    no pixel refers to, a mesh table of static entries), so the ring's slots grow."""
    hits = np.zeros((h, w), dtype=_lib.HIT_DTYPE)
    ys, xs = np.mgrid[0:h, 0:w]
    hits["kind"], hits["mesh"], hits["t"], hits["normal"] = 1, 0xFFFFFFFF, 4.0, (0.0, 0.6, 0.8)
    hits["index"] = (xs // 32 + 2 * (ys // 32)) % 4
    rng = np.random.default_rng(seed)
    px = 4.0 * 2.0 / h  # one pixel at the guide's depth
    chain = []
    for k in range(calls):
        shifts = rng.integers(-1, 2, (4, 2))
        shifts[shifts.any(1) == 0] = (1, -1)  # every sphere moves in every call
        moving = [(pose(None, (0.0, dy * px, dz * px)), M.MOVING) for dy, dz in shifts]
        pad = [(np.full(12, 7.0, F32), 0)] * int(rng.integers(0, 40) + 300 * (k % 5 == 2))
        chain.append((M.table(moving + pad), M.static(int(rng.integers(0, 9))) if k % 3 else None))
    return hits, chain


def lifetime_chain(acc, cnt, mom, view, hits, chain, moments, skip=None):
    """The numpy chain of lifetime_inputs' calls (NEAREST, thresholds that reject no depth or normal); skip: the call
    whose spheres table is replaced by a static one."""
    for k, (spheres, meshes) in enumerate(chain):
        args = (view, hits, view, hits, M.static(len(spheres)) if k == skip else spheres, meshes, H.NEAREST, 1e30, -2.0)
        if moments:
            acc, cnt, mom = M.reproject_moments(acc, cnt, mom, *args)
        else:
            acc, cnt = M.reproject(acc, cnt, *args)
    return acc, cnt, mom


@pytest.mark.parametrize("moments", [False, True])
def test_tables_are_copied_before_the_call_returns(moments):
    """Twelve back-to-back calls -- three times the ring's depth -- with no synchronise between them, each with its own
    tables, which are overwritten with garbage as soon as the call has returned.  The history survives all twelve, and
    the final state depends on each single call's table (asserted on the restatement: a static table in place of any
    one of them changes the expected state), so a slot reused too early, a wrong slot uploaded or tables mixed between
    calls cannot pass."""
    size = w, h = (64, 64)
    mode = _lib.MODE_RGBA32F
    calls = 3 * _lib.MOTION_RING
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context(mode=mode, debug=True)
    src = synthetic_source(w, h, mode)
    hits, chain = lifetime_inputs(w, h, calls)
    d_hits = DevBuf(w * h * 32).write(hits)
    _, view, _ = view_pairs(size)[0]
    _, _, mom = traced_moments(ctx, case, (3, 4))
    ctx.load_accumulator(src)
    ctx.fill_history(5)
    cnt = np.full((h, w), 5, np.uint32)
    want = lifetime_chain(src, cnt, mom, view.record, hits, chain, moments)
    assert (want[1] > 0).mean() > 0.25  # history is left to compare
    for k in range(calls):
        other = lifetime_chain(src, cnt, mom, view.record, hits, chain, moments, skip=k)
        assert not (np.array_equal(other[1], want[1]) and equal(other[0], want[0])), k
    ctx.synchronize()
    for spheres, meshes in chain:
        mine = [None if t is None else t.copy() for t in (spheres, meshes)]
        call(ctx, view, d_hits.ptr, view, d_hits.ptr, mine[0], mine[1], moments, filter=_lib.REPROJECT_NEAREST,
             depth_tolerance=1e30, min_normal_dot=-2.0)
        for t in mine:  # garbage over the caller's arrays right after the call
            if t is not None:
                t.view(np.uint8)[:] = 0xFF
    check(ctx, mode, want[0], want[1], want[2] if moments else None, "chain")
    assert ctx.check_guards()[1] == 0
    ctx.close()
    d_hits.free()


# ---- 5. the rejections -------------------------------------------------------------------------------------------------------

def test_rejections_enqueue_nothing_and_leave_the_context_usable():
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context()
    ctx.trace(case.push(1))
    ctx.accumulate_history_moments(4)
    lib, handle = ctx.lib, ctx.handle
    d_hits = DevBuf(w * h * 32)
    ctx.intersect_primary_into(case.push(), d_hits.ptr)
    view = E.View(case.camera, size, case.settings)
    good = ctx.reproject_info()
    acc, cnt, mom, accumulates = ctx.read(ACCUM), ctx.read_history(), ctx.read_moments(), ctx.stats().accumulates
    ok = M.table([(pose(rotation([0, 0, 1], 0.1), [0.1, 0, 0]), M.MOVING), (IDENTITY, 0)])

    def bad_entry(i, value, flags=M.MOVING):
        t = ok.copy()
        t["m"][0, i], t["flags"][0] = value, flags
        return t

    for fn, who in ((lib.hrt_reproject_motion, b"hrt_reproject_motion: "),
                    (lib.hrt_reproject_motion_moments, b"hrt_reproject_motion_moments: ")):
        def raw(tables, info=good):
            return fn(handle, ctypes.byref(info), ctypes.byref(tables) if tables is not None else None,
                      ctypes.byref(view.record), ctypes.c_void_p(d_hits.ptr), ctypes.byref(view.record),
                      ctypes.c_void_p(d_hits.ptr))

        def refused(tables, word):
            assert raw(tables) == 1, word
            msg = lib.hrt_last_error(handle)
            assert msg.startswith(who) and word in msg, (word, msg)

        refused(None, b"null motion")
        big = M.static(M.MAX_OBJECTS + 1)
        refused(tables_arg(big, None), b"HRT_MOTION_MAX_OBJECTS")
        refused(tables_arg(None, big), b"HRT_MOTION_MAX_OBJECTS")
        refused(_lib.MotionTables(None, 1, None, 0), b"null pointer")
        refused(_lib.MotionTables(None, 0, None, 2), b"null pointer")
        refused(tables_arg(bad_entry(0, 1.0, 2), None), b"flag")
        refused(tables_arg(None, bad_entry(0, 1.0, 0x80000001)), b"flag")
        for i, v in ((0, np.nan), (11, np.inf), (5, -np.inf)):
            refused(tables_arg(bad_entry(i, v), None), b"finite")
            refused(tables_arg(ok, bad_entry(i, v)), b"finite")
        assert raw(tables_arg(bad_entry(3, np.nan, 0), None)) == 0  # a static entry's matrix is not looked at
        acc, cnt, mom = ctx.read(ACCUM), ctx.read_history(), ctx.read_moments()  # (identical views: what that pass left)
        # an existing rejection still names the new call
        info = ctx.reproject_info()
        info.filter = 2
        assert raw(tables_arg(ok, ok), info) == 1 and lib.hrt_last_error(handle).startswith(who + b"unknown filter")
    assert ctx.read(ACCUM).tobytes() == acc.tobytes() and ctx.read_history().tobytes() == cnt.tobytes()
    assert ctx.read_moments().tobytes() == mom.tobytes() and ctx.stats().accumulates == accumulates
    call(ctx, view, d_hits.ptr, view, d_hits.ptr, ok, ok, True)  # still usable
    ctx.synchronize()
    ctx.close()
    assert lib.hrt_reproject_motion(None, ctypes.byref(good), None, None, None, None, None) == 1
    parts = [case.context(partition=(8, p, 2)) for p in range(2)]
    for c in parts:
        with pytest.raises(_lib.HrtError, match="partition"):
            call(c, view, d_hits.ptr, view, d_hits.ptr, ok, ok, False)
        c.close()
    single = case.context()
    E.HrtContext.comm_init_all([single])
    with pytest.raises(_lib.HrtError, match="communicator"):
        call(single, view, d_hits.ptr, view, d_hits.ptr, ok, ok, True)
    single.close()
    d_hits.free()


# ---- 6. nothing else moves ---------------------------------------------------------------------------------------------------

def _stats_tuple(st):
    return (st.segments, st.tri_tests, st.traces, st.last_kernel, st.last_block, st.last_frames, st.accumulates)


@pytest.mark.parametrize("mode", MODES)
def test_the_old_entry_points_give_the_same_bytes_before_and_after(mode):
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    opts = {_lib.OPT_FOLD_RECORDS: 1}
    ctx, twin = case.context(mode=mode, debug=True, options=opts), case.context(mode=mode, options=opts)
    hits = synthetic_guide(w, h)
    d_hits = DevBuf(w * h * 32).write(hits)
    target = DevBuf(w * h * 4)
    _, prev, cur = view_pairs(size)[1]
    _, spheres, meshes = synthetic_tables(2.0 / h, 3)[0]

    def old_calls(c, base):
        for frame in range(3):
            c.trace(case.push(base + frame))
            c.accumulate(frame)
        c.compute_n(case.push(base + 5), 2)
        c.fill_history(3)
        c.fill_moments(0.25, 0.5)
        c.trace(case.push(base + 9))
        c.accumulate_history_moments(8)
        c.reproject_moments(prev, d_hits.ptr, cur, d_hits.ptr)
        c.reproject(cur, d_hits.ptr, prev, d_hits.ptr, filter=_lib.REPROJECT_NEAREST)

    def state(c):
        return (c.read(ACCUM, native(mode)).tobytes(), c.read_history().tobytes(), c.read_moments().tobytes(),
                c.read(TRACE, native(mode)).tobytes(), _stats_tuple(c.stats()), c.fold_records(with_total=True)[1],
                c.fold_records(with_total=True)[0].tobytes())

    for c in (ctx, twin):
        old_calls(c, 1)
    assert state(ctx) == state(twin)
    t_ctx, t_twin = (c.present(ACCUM, target.ptr, target.nbytes, w, h) for c in (ctx, twin))
    before = state(ctx)
    call(ctx, prev, d_hits.ptr, cur, d_hits.ptr, spheres, meshes, True)
    call(ctx, cur, d_hits.ptr, prev, d_hits.ptr, spheres, meshes, False, filter=_lib.REPROJECT_NEAREST)
    after = state(ctx)
    # the trace image, hrt_stats (accumulates included: hrt_reproject leaves it too) and the fold records stay
    assert after[3:] == before[3:] and after[:2] != before[:2]
    assert ctx.present(ACCUM, target.ptr, target.nbytes, w, h) == t_ctx + 1  # no ticket was issued in between
    assert twin.present(ACCUM, target.ptr, target.nbytes, w, h) == t_twin + 1
    for c in (ctx, twin):
        c.load_accumulator(np.frombuffer(before[0], np.uint8 if mode == _lib.MODE_RGBA8 else F32).reshape(h, w, 4).copy())
        old_calls(c, 20)
    assert state(ctx) == state(twin)
    ctx.synchronize()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    d_hits.free()
    target.free()


# ---- 7. the mirrors ------------------------------------------------------------------------------------------------------------

def _write_scene(path, settings):
    with open(path, "wb") as f:
        f.write(np.uint32(len(settings.sphere_data)).tobytes())
        for s in settings.sphere_data:
            f.write(np.float32([*s.centre, s.radius]).tobytes())
        f.write(np.uint32(len(settings.mesh_data)).tobytes())
        for m in settings.mesh_data:
            f.write(np.uint32([len(m.mesh.positions), len(m.mesh.indices)]).tobytes())
            f.write(np.asarray(m.mesh.positions, F32).tobytes())
            f.write(np.asarray(m.mesh.indices, np.uint32).tobytes())


def test_python_and_cpp_mirrors(tmp_path):
    """DiffusePipeline.reproject_history(motion=...), HrtContext.reproject_motion with record lists and E.motion_between
    against the numpy chain; include/hrt_app.hpp's motion_between / Context::reproject_motion_moments
    (tests/cpp/motion_demo) against the Python mirror's bytes: the box scene's geometry, its sphere slid sideways."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "motion_demo.mk"], check=True)  # (up to date after build())
    _, settings = E.preset("box")
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    _write_scene(src, settings)
    r = subprocess.run([os.path.join(cpp, "motion_demo"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    size = w, h = 48, 32
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [w, h] and len(raw) == 8 + w * h * (4 + 8 + 16)
    got_cnt = np.frombuffer(raw[8:8 + w * h * 4], np.uint32).reshape(h, w)
    got_mom = np.frombuffer(raw[8 + w * h * 4:8 + w * h * 12], F32).reshape(h, w, 2)
    got_acc = np.frombuffer(raw[8 + w * h * 12:], F32).reshape(h, w, 4)
    # the same through the Python mirror and the numpy chain
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    shift = (0.0, 0.05, 0.3)

    def scene(moved):
        spheres = [E.Sphere([float(F32(F32(c) + F32(d if moved else 0.0))) for c, d in zip(s.centre, shift)], s.radius, grey)
                   for s in settings.sphere_data]
        return E.RayTracerSettings(num_samples=1, max_bounces=4, use_environment_lighting=True, sphere_data=spheres,
                                   mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in settings.mesh_data])

    ctx = E.HrtContext(size, device=0, mode=_lib.MODE_RGBA32F)
    cam = E.Camera([1.5, 1.0, 0.0], [-1.0, 0.0, 0.0])
    pipe, diffuse = E.RayTracePipeline(ctx, size, scene(False)), E.DiffusePipeline(ctx, size)
    acc, cnt, mom = np.zeros((h, w, 4), F32), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    for frame in range(3):
        pipe.compute(cam, frame)
        diffuse.next_frame_history(pipe.image(), moments=True)
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, ctx.read(TRACE, RGBA32F), 32)
    d_hits = [DevBuf(w * h * 32), DevBuf(w * h * 32)]
    pipe.first_hits_into(cam, d_hits[0].ptr)
    pipe = E.RayTracePipeline(ctx, size, scene(True))  # hrt_set_scene with the sphere moved
    pipe.first_hits_into(cam, d_hits[1].ptr)
    hp, hc = (d.read().view(_lib.HIT_DTYPE).reshape(h, w) for d in d_hits)
    view = E.View(cam, size, scene(True))
    rec = E.motion_between(pose(None, (0, 0, 0)), pose(None, shift))
    diffuse.reproject_history(view, d_hits[0].ptr, view, d_hits[1].ptr, motion=([rec], None), moments=True)
    spheres = M.table([M.motion_between(pose(None, (0, 0, 0)), pose(None, shift))])
    acc, cnt, mom = M.reproject_moments(acc, cnt, mom, view.record, hp, view.record, hc, spheres, None, H.BILINEAR, *H.DEFAULTS)
    pipe.compute(cam, 3)
    diffuse.next_frame_history(pipe.image(), moments=True)
    acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, ctx.read(TRACE, RGBA32F), 32)
    check_state(ctx, _lib.MODE_RGBA32F, acc, cnt, mom, "python mirror")
    assert (hc["kind"] == 1).sum() > 20 and (cnt[hc["kind"] == 1] > 1).mean() > 0.5  # the sphere kept its history
    assert equal(got_cnt, cnt) and equal(got_mom, mom) and equal(got_acc, acc), report(got_acc, acc)
    ctx.close()
    for d in d_hits:
        d.free()
