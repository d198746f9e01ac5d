"""Temporal history on the device (hrt_reproject, hrt_accumulate_history, hrt_fill_history, hrt_read_history;
DESIGN.md §2 S15, §28): every byte of the accumulator and of the count image against the numpy restatement of
S15 (tests/history_ref.py), NaN compared as NaN.  Accumulators are loaded (bytes; floats above 1, NaN and
infinite texels), the frames folded in are traced, counts come from hrt_fill_history and from the rejections of
earlier reprojections, guides are synthetic or the real first hits of box and spheres on either side of a real
camera move.  Then the properties of the calls (what they leave alone, guard bands, the old entry points
before and after), the rejections, and the Python and C++ mirrors."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import history_ref as H
from helpers import E, SceneCase, _lib
from image_ref import same_floats

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = np.finfo(F32).max
FILL = 0xA5
TRACE, ACCUM = _lib.IMG_TRACE, _lib.IMG_ACCUM
RGBA8, RGBA32F = _lib.FMT_RGBA8, _lib.FMT_RGBA32F
MODES = [_lib.MODE_RGBA8, _lib.MODE_RGBA32F]
FILTERS = [_lib.REPROJECT_NEAREST, _lib.REPROJECT_BILINEAR]
SIZES = [(1, 1), (2, 2), (37, 23), (64, 64), (130, 70)]  # (width, height)
CAP = 1 << 24
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        _hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.hipFree.argtypes = [ctypes.c_void_p]
    return _hip


class DevBuf:
    """nbytes of device memory filled with 0xA5."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        assert hip().hipMalloc(ctypes.byref(p), nbytes) == 0
        self.ptr, self.nbytes = int(p.value), nbytes
        assert hip().hipMemset(self.ptr, FILL, self.nbytes) == 0 and hip().hipDeviceSynchronize() == 0

    def write(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes and hip().hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0
        return self

    def read(self):
        out = np.empty(self.nbytes, np.uint8)
        assert hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return out

    def free(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = 0


def native(mode):
    return RGBA8 if mode == _lib.MODE_RGBA8 else RGBA32F


def equal(got, want):
    if want.dtype != F32:
        return got.tobytes() == want.tobytes()
    return bool(same_floats(got, want).all())


def report(got, want):
    same = same_floats(got, want) if want.dtype == F32 else got == want
    bad = np.argwhere(~same.reshape(same.shape[0], same.shape[1], -1).all(-1))
    y, x = bad[0]
    return f"{len(bad)} pixels differ; first at (x={x}, y={y}): {got[y, x]} vs {want[y, x]}"


def check_state(ctx, mode, acc, cnt, what):
    got = ctx.read(ACCUM, native(mode))
    assert equal(got, acc), (what, "accumulator", report(got, acc))
    got = ctx.read_history()
    assert equal(got, cnt), (what, "counts", report(got, cnt))


# ---- inputs --------------------------------------------------------------------------------------------------

def synthetic_source(w, h, mode, seed=1):
    """A loadable accumulator: random bytes, or random floats in [0, 4) with a few NaN and infinite texels."""
    rng = np.random.default_rng([seed, w, h])
    if mode == _lib.MODE_RGBA8:
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img = (rng.uniform(0, 1, (h, w, 4)) ** 2 * 4).astype(F32)
    n = w * h
    if n >= 15:
        flat = img.reshape(n, 4)
        at = rng.choice(n, 3, replace=False)
        flat[at[0], 0], flat[at[1], 2], flat[at[2], 1] = np.nan, np.inf, -np.inf
    return img


def synthetic_guide(w, h, seed=2):
    """Blocky random keys with misses, sphere and triangle keys; normals on and off the unit sphere; depths with
    equal values; FLT_MAX, zero and NaN depths on surfaces; one NaN normal."""
    rng = np.random.default_rng([seed, w, h])
    hits = np.zeros((h, w), dtype=_lib.HIT_DTYPE)
    by, bx = np.mgrid[0:h, 0:w]
    block = rng.integers(0, 6, ((h + 6) // 7, (w + 8) // 9))[by // 7, bx // 9]
    hits["kind"] = np.choose(block % 3, [0, 1, 2])
    hits["index"] = np.where(hits["kind"] == 0, 0xFFFFFFFF, block + 3)
    hits["mesh"] = np.where(hits["kind"] == 2, block // 3, 0xFFFFFFFF)
    n = rng.normal(size=(h, w, 3))
    unit = n / np.linalg.norm(n, axis=-1, keepdims=True)
    smooth = np.broadcast_to(np.array([0.0, 0.6, 0.8]), (h, w, 3)) + rng.normal(size=(h, w, 3)) * 0.05
    hits["normal"] = np.where((rng.uniform(size=(h, w)) < 0.7)[..., None], smooth, unit * rng.uniform(0.5, 2, (h, w, 1)))
    t = np.round(rng.uniform(2, 6, (h, w)) * 4) / 4  # many equal depths
    r = rng.uniform(size=(h, w))
    t[r < 0.03] = FLT_MAX
    t[(r >= 0.03) & (r < 0.06)] = 0.0
    t[(r >= 0.06) & (r < 0.09)] = np.nan
    hits["t"] = np.where(hits["kind"] == 0, FLT_MAX, t)
    if w * h >= 15:
        hits["normal"][h // 2, w // 2] = (np.nan, 0.0, 1.0)
    return hits


def turned(cam, dpos, turn):
    d = np.asarray(cam.direction, np.float64)
    d /= np.linalg.norm(d)
    up = np.asarray(cam.up, np.float64)
    side = np.cross(d, up)
    side /= np.linalg.norm(side)
    nd = d + turn[0] * side + turn[1] * up
    return E.Camera([float(F32(a + b)) for a, b in zip(cam.position, dpos)], [float(F32(v)) for v in nd], cam.up)


def view_pairs(size):
    """(name, prev, cur) views: identity; a turn of a few pixels; a previous camera ahead of the current one and
    turned far enough that some surface points lie behind it; a previous grid with zero dx."""
    cam, settings = E.preset("box")
    base = E.View(cam, size, settings)
    px = 2.0 / size[1]
    turn = E.View(turned(cam, (0.0, 0.0, 0.0), (2.5 * px, -1.25 * px)), size, settings)
    ahead = E.View(turned(cam, (-3.0, 0.2, 0.4), (1.4, 0.1)), size, settings)
    flat = copy.deepcopy(base)
    flat.record.grid_dx[:] = [0.0, 0.0, 0.0, 0.0]
    return [("identity", base, base), ("turn", base, turn), ("behind", ahead, base), ("zero dx", flat, base)]


# ---- 1. the history fold ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_fold_with_per_pixel_counts(size, mode):
    w, h = size
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context(mode=mode, debug=True)
    ctx.trace(case.push(1))
    new = ctx.read(TRACE, native(mode))
    src = synthetic_source(w, h, mode)
    assert (ctx.read_history() == 0).all()  # allocated and zeroed by the first call
    # uniform counts: none, one, below / at the cap, the largest cap, and the count whose successor wraps
    for count, cap in ((0, 32), (1, 32), (31, 32), (32, 32), (40, 32), (CAP - 1, CAP), (CAP, CAP), (2**32 - 1, CAP),
                       (5, 1)):
        ctx.load_accumulator(src)
        ctx.fill_history(count)
        cnt = np.full((h, w), count, np.uint32)
        check_state(ctx, mode, src, cnt, ("fill", count))
        ctx.accumulate_history(cap)
        acc, cnt = H.accumulate_history(src, cnt, new, cap)
        check_state(ctx, mode, acc, cnt, ("fold", count, cap))
        assert (cnt == min(count + 1, cap)).all()
    # mixed counts: what a reprojection with rejections leaves, folded twice
    hits = synthetic_guide(w, h)
    other = hits.copy()
    other["kind"][::2, 1::3] = 0
    d_prev, d_cur = DevBuf(w * h * 32).write(other), DevBuf(w * h * 32).write(hits)
    view = view_pairs(size)[0][1]
    ctx.load_accumulator(src)
    ctx.fill_history(6)
    ctx.reproject(view, d_prev.ptr, view, d_cur.ptr, filter=_lib.REPROJECT_NEAREST, depth_tolerance=0.5)
    acc, cnt = H.reproject(src, np.full((h, w), 6, np.uint32), view.record, other, view.record, hits, H.NEAREST, 0.5)
    check_state(ctx, mode, acc, cnt, "mixed")
    if w * h >= 15:
        assert set(np.unique(cnt)) == {0, 6}
    for cap in (32, 7):
        ctx.trace(case.push(2 + cap))
        new = ctx.read(TRACE, native(mode))
        ctx.accumulate_history(cap)
        acc, cnt = H.accumulate_history(acc, cnt, new, cap)
        check_state(ctx, mode, acc, cnt, ("mixed fold", cap))
    buffers, corrupted = ctx.check_guards()
    assert buffers > 0 and corrupted == 0
    ctx.close()
    d_prev.free()
    d_cur.free()


# ---- 2. the reprojection of synthetic accumulators, counts and guides --------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_reprojection_of_synthetic_history(size, mode):
    w, h = size
    ctx = E.HrtContext(size, device=0, mode=mode, debug=True)
    src = synthetic_source(w, h, mode)
    prev_hits, cur_hits = synthetic_guide(w, h, seed=2), synthetic_guide(w, h, seed=2)
    rng = np.random.default_rng([7, w, h])
    change = rng.uniform(size=(h, w)) < 0.15  # the previous view saw another surface, depth or normal there
    prev_hits["mesh"][change & (prev_hits["kind"] == 2)] += 1
    prev_hits["t"][change & (prev_hits["kind"] == 1)] *= F32(1.01)
    d_prev, d_cur = DevBuf(w * h * 32).write(prev_hits), DevBuf(w * h * 32).write(cur_hits)
    guarded = None
    for name, prev, cur in view_pairs(size):
        if name == "behind" and w * h >= 15:
            _, _, ok, _, _ = H.source_coords(prev.record, cur.record, cur_hits)
            assert ok.any() and not ok.all()  # some pixels are behind the previous camera
        for filt in FILTERS:
            for tol, mind in (H.DEFAULTS, (0.0, -2.0), (1e30, -2.0), (0.5, 0.99)):
                # counts: uniform, then whatever the reprojection and one fold of the cleared trace image leave
                ctx.load_accumulator(src)
                ctx.fill_history(CAP if filt == _lib.REPROJECT_NEAREST else 9)
                acc = src
                cnt = np.full((h, w), CAP if filt == _lib.REPROJECT_NEAREST else 9, np.uint32)
                for rep in range(2):
                    ctx.reproject(prev, d_prev.ptr, cur, d_cur.ptr, filter=filt, depth_tolerance=tol, min_normal_dot=mind)
                    acc, cnt = H.reproject(acc, cnt, prev.record, prev_hits, cur.record, cur_hits, filt, tol, mind)
                    check_state(ctx, mode, acc, cnt, (name, filt, tol, mind, rep))
                    if rep == 0:
                        ctx.trace(_lib.PushConstants(init=1, width=w, height=h))
                        new = ctx.read(TRACE, native(mode))
                        ctx.accumulate_history(CAP)
                        acc, cnt = H.accumulate_history(acc, cnt, new, CAP)
                        check_state(ctx, mode, acc, cnt, (name, filt, tol, mind, "fold"))
                if name == "zero dx":
                    assert (cnt == 0).all()
                if name == "identity" and tol > 1 and filt == _lib.REPROJECT_NEAREST and w * h >= 15:
                    assert len(np.unique(cnt)) >= 2  # mixed counts went through the second reprojection
                now = ctx.check_guards()
                assert now[1] == 0 and (guarded is None or now[0] == guarded)  # the buffers are reused
                guarded = now[0]
    assert d_prev.read().tobytes() == prev_hits.tobytes() and d_cur.read().tobytes() == cur_hits.tobytes()
    ctx.close()
    d_prev.free()
    d_cur.free()


# ---- 3. traced frames, real first hits, a real move; and what the calls leave alone -----------------------------

def _stats_tuple(st):
    # (timings and wave_steps depend on scheduling: tests/test_gpu_intersect.py)
    return (st.segments, st.tri_tests, st.traces, st.last_kernel, st.last_block, st.last_frames)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,size", [("box", (64, 64)), ("spheres", (130, 70))])
def test_four_frame_chain_across_real_moves(name, size, mode):
    w, h = size
    case = SceneCase(name, size, num_samples=1, max_bounces=4)
    ctx = case.context(mode=mode, debug=True, options={_lib.OPT_FOLD_RECORDS: 1})
    px = 2.0 / h
    cams = [case.camera]
    for k in range(3):
        cams.append(turned(cams[-1], (0.03, 0.01 * k, 0.02), (1.5 * px * (k + 1), -0.75 * px)))
    d_hits = [DevBuf(w * h * 32), DevBuf(w * h * 32)]
    target = DevBuf(w * h * 4)
    t0 = ctx.present(ACCUM, target.ptr, target.nbytes, w, h)
    records = ctx.fold_records(with_total=True)
    acc = np.zeros((h, w, 4), np.uint8 if mode == _lib.MODE_RGBA8 else F32)
    acc[..., 3] = 255 if mode == _lib.MODE_RGBA8 else 1.0
    cnt = np.zeros((h, w), np.uint32)
    hits = view = None
    for k, cam in enumerate(cams):
        case.camera = cam
        cur_view = E.View(cam, size, case.settings)
        ctx.intersect_primary_into(case.push(), d_hits[k & 1].ptr)
        cur_hits = d_hits[k & 1].read().view(_lib.HIT_DTYPE).reshape(h, w)
        ctx.trace(case.push(1 + k))
        new = ctx.read(TRACE, native(mode))
        stats, accumulates = _stats_tuple(ctx.stats()), ctx.stats().accumulates
        if k:
            filt = FILTERS[k & 1]
            ctx.reproject(view, d_hits[(k - 1) & 1].ptr, cur_view, d_hits[k & 1].ptr, filter=filt)
            acc, cnt = H.reproject(acc, cnt, view.record, hits, cur_view.record, cur_hits, filt, *H.DEFAULTS)
            check_state(ctx, mode, acc, cnt, (k, "reproject"))
            kept = float((cnt > 0).mean())
            assert 0.5 < kept < 1.0, kept  # the move carries most of the history, not all of it
            assert ctx.stats().accumulates == accumulates
        ctx.accumulate_history(32)
        acc, cnt = H.accumulate_history(acc, cnt, new, 32)
        check_state(ctx, mode, acc, cnt, (k, "fold"))
        # the trace image, the hit arrays and everything in hrt_stats but `accumulates` are as they were
        assert ctx.read(TRACE, native(mode)).tobytes() == new.tobytes()
        assert d_hits[k & 1].read().tobytes() == cur_hits.tobytes()
        assert _stats_tuple(ctx.stats()) == stats and ctx.stats().accumulates == accumulates + 1
        hits, view = cur_hits, cur_view
    assert set(np.unique(cnt)) <= {1, 2, 3, 4} and len(np.unique(cnt)) >= 3
    # no fold record was appended, no ticket issued
    after = ctx.fold_records(with_total=True)
    assert after[1] == records[1] and after[0].tobytes() == records[0].tobytes()
    assert ctx.present(ACCUM, target.ptr, target.nbytes, w, h) == t0 + 1
    # the pipeline's last stage: the denoise pass over the history, guided by the current first hits
    got = ctx.denoise(RGBA32F, d_hits[(len(cams) - 1) & 1].ptr)
    want = D.denoise(acc, 5, D.DEFAULT_SIGMAS, hits)
    assert equal(got, want), report(got, want)
    ctx.synchronize()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    for b in d_hits + [target]:
        b.free()


@pytest.mark.parametrize("mode", MODES)
def test_the_old_entry_points_give_the_same_bytes_before_and_after(mode):
    """hrt_accumulate, hrt_compute_n and the deferred combiner on a context that used the history calls (whose
    reprojection swapped the accumulator's buffer) against a twin that never did."""
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, debug=True), case.context(mode=mode)
    for c in (ctx, twin):
        for frame in range(3):
            c.trace(case.push(1 + frame))
            c.accumulate(frame)
    saved = twin.read(ACCUM, native(mode))
    assert ctx.read(ACCUM, native(mode)).tobytes() == saved.tobytes()
    hits = synthetic_guide(w, h)
    d_hits = DevBuf(w * h * 32).write(hits)
    view = view_pairs(size)[1]
    ctx.fill_history(3)
    ctx.reproject(view[1], d_hits.ptr, view[2], d_hits.ptr)
    ctx.accumulate_history(8)
    ctx.reproject(view[2], d_hits.ptr, view[1], d_hits.ptr, filter=_lib.REPROJECT_NEAREST)
    assert ctx.read(ACCUM, native(mode)).tobytes() != saved.tobytes()
    counts = ctx.read_history()
    ctx.load_accumulator(saved)
    for c in (ctx, twin):
        c.trace(case.push(4))
        c.accumulate(3)
        c.compute_n(case.push(5), 3)
        c.set_option(_lib.OPT_DEFER_COMBINE, 1)
        for frame in range(6, 9):
            c.trace(case.push(1 + frame))
            c.accumulate(frame)
    assert ctx.read(ACCUM, native(mode)).tobytes() == twin.read(ACCUM, native(mode)).tobytes()
    assert ctx.read_history().tobytes() == counts.tobytes()  # none of them touched the count image
    # with combines deferred: the pending fold first, then the history fold of the newest trace
    for c in (ctx, twin):
        c.trace(case.push(20))
        c.accumulate(9)
    acc9 = twin.read(ACCUM, native(mode))
    ctx.trace(case.push(21))
    new = ctx.read(TRACE, native(mode))
    ctx.accumulate_history(8)
    acc, cnt = H.accumulate_history(acc9, counts, new, 8)
    check_state(ctx, mode, acc, cnt, "deferred")
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    d_hits.free()


# ---- 4. hrt_fill_history / hrt_read_history -----------------------------------------------------------------------

def test_fill_and_read_round_trips_host_and_device():
    size = w, h = (37, 23)
    ctx = E.HrtContext(size, device=0, debug=True)
    dev = DevBuf(w * h * 4 + 64)
    for count in (0, 1, 77, CAP, 2**32 - 1):
        ctx.fill_history(count)
        assert (ctx.read_history() == count).all()
        ctx.read_history_into(dev.ptr, w * h * 4)
        raw = dev.read()
        assert (raw[:w * h * 4].view(np.uint32) == count).all() and (raw[w * h * 4:] == FILL).all()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    dev.free()


# ---- 5. the rejections ---------------------------------------------------------------------------------------------

def test_rejections_enqueue_nothing_and_leave_the_context_usable():
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context()
    ctx.trace(case.push(1))
    ctx.accumulate_history(4)
    lib, handle = ctx.lib, ctx.handle
    d_hits = DevBuf(w * h * 32 + 16)
    ctx.intersect_primary_into(case.push(), d_hits.ptr)
    view = E.View(case.camera, size, case.settings).record
    good = ctx.reproject_info()
    acc, cnt, accumulates = ctx.read(ACCUM), ctx.read_history(), ctx.stats().accumulates
    host_raw = np.zeros(w * h * 32 + 16, np.uint8)
    host_hits = host_raw.ctypes.data + (-host_raw.ctypes.data) % 16  # aligned, but pageable host memory

    def raw(info=good, prev=view, prev_hits=d_hits.ptr, cur=view, cur_hits=d_hits.ptr):
        ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
        return lib.hrt_reproject(handle, ref(info), ref(prev), ctypes.c_void_p(prev_hits or 0), ref(cur),
                                 ctypes.c_void_p(cur_hits or 0))

    def altered(**kw):
        info = ctx.reproject_info()
        for k, v in kw.items():
            setattr(info, k, v)
        return info

    for kw in (dict(info=None), dict(prev=None), dict(cur=None), dict(prev_hits=None), dict(cur_hits=None)):
        assert raw(**kw) == 1 and b"null" in lib.hrt_last_error(handle), kw
    for field, value, word in (("filter", 2, b"filter"), ("flags", 1, b"flags"), ("depth_tolerance", -0.01, b"tolerance"),
                               ("depth_tolerance", float("nan"), b"tolerance"), ("depth_tolerance", float("inf"), b"tolerance"),
                               ("min_normal_dot", float("nan"), b"min_normal_dot"),
                               ("min_normal_dot", float("-inf"), b"min_normal_dot")):
        assert raw(info=altered(**{field: value})) == 1 and word in lib.hrt_last_error(handle), (field, value)
    for which in ("prev_hits", "cur_hits"):
        assert raw(**{which: host_hits}) == 1 and b"device" in lib.hrt_last_error(handle)            # host memory
        assert raw(**{which: d_hits.ptr + 8}) == 1 and b"aligned" in lib.hrt_last_error(handle)        # misaligned
    for bad in (0, CAP + 1, 2**32 - 1):
        assert lib.hrt_accumulate_history(handle, bad) == 1 and b"max_history" in lib.hrt_last_error(handle)
    small = np.full(w * h, 7, np.uint32)
    assert lib.hrt_read_history(handle, _lib.ptr(small), small.nbytes - 1) == 1 and b"too small" in lib.hrt_last_error(handle)
    assert lib.hrt_read_history(handle, None, small.nbytes) == 1 and b"null" in lib.hrt_last_error(handle)
    assert (small == 7).all()
    # nothing was enqueued: accumulator, counts and statistics are as they were, and the calls still work
    assert ctx.read(ACCUM).tobytes() == acc.tobytes() and ctx.read_history().tobytes() == cnt.tobytes()
    assert ctx.stats().accumulates == accumulates
    ctx.reproject_info(depth_tolerance=0.0, min_normal_dot=-2.0)  # the edges of the accepted ranges
    assert raw(info=altered(depth_tolerance=0.0, min_normal_dot=-2.0)) == 0
    ctx.accumulate_history(CAP)
    ctx.close()
    # a row-tile partition, with and without a communicator, and an unpartitioned context joined to one
    parts = [case.context(partition=(8, p, 2)) for p in range(2)]
    view_py = E.View(case.camera, size, case.settings)
    for joined in (False, True):
        if joined:
            E.HrtContext.comm_init_all(parts)
        for c in parts:
            for call in (lambda: c.reproject(view_py, d_hits.ptr, view_py, d_hits.ptr), lambda: c.accumulate_history(4),
                         lambda: c.fill_history(1), c.read_history):
                with pytest.raises(_lib.HrtError, match="partition"):
                    call()
    for c in parts:
        c.close()
    single = case.context()
    E.HrtContext.comm_init_all([single])
    with pytest.raises(_lib.HrtError, match="communicator"):
        single.accumulate_history(4)
    with pytest.raises(_lib.HrtError, match="communicator"):
        single.reproject(view_py, d_hits.ptr, view_py, d_hits.ptr)
    single.close()
    d_hits.free()


# ---- 6. the mirrors --------------------------------------------------------------------------------------------------

def _demo_sequence(settings, size, mode):
    """What tests/cpp/history_demo.cpp does, through the Python mirror: (counts after the reprojection, counts and
    accumulator after the last fold, and the numpy chain's)."""
    w, h = size
    ctx = E.HrtContext(size, device=0, mode=mode)
    pipe, diffuse = E.RayTracePipeline(ctx, size, settings), E.DiffusePipeline(ctx, size)
    before, after = E.Camera(), E.Camera([0.05, 0.02, -0.03], [1.0, 0.03, 0.08])
    acc, cnt = np.zeros((h, w, 4), F32), np.zeros((h, w), np.uint32)
    for frame in range(3):
        pipe.compute(before, frame)
        diffuse.next_frame_history(pipe.image())
        acc, cnt = H.accumulate_history(acc, cnt, ctx.read(TRACE, RGBA32F), 32)
    d_hits = [DevBuf(w * h * 32), DevBuf(w * h * 32)]
    pipe.first_hits_into(before, d_hits[0].ptr)
    pipe.first_hits_into(after, d_hits[1].ptr)
    hp, hc = (d.read().view(_lib.HIT_DTYPE).reshape(h, w) for d in d_hits)
    vp, vc = E.View(before, size, settings), E.View(after, size, settings)
    ctx.reproject(vp, d_hits[0].ptr, vc, d_hits[1].ptr)
    acc, cnt = H.reproject(acc, cnt, vp.record, hp, vc.record, hc, H.BILINEAR, *H.DEFAULTS)
    carried = ctx.read_history()
    assert equal(carried, cnt) and 0 < (cnt == 0).sum() < cnt.size
    pipe.compute(after, 3)
    diffuse.next_frame_history(pipe.image())
    acc, cnt = H.accumulate_history(acc, cnt, ctx.read(TRACE, RGBA32F), 32)
    out = carried, ctx.read_history(), ctx.read(ACCUM, RGBA32F)
    assert equal(out[1], cnt) and equal(out[2], acc), report(out[2], acc)
    ctx.close()
    for d in d_hits:
        d.free()
    return out


def test_python_and_cpp_mirrors(tmp_path):
    """E.View, HrtContext.reproject / read_history and DiffusePipeline.next_frame_history against the numpy chain,
    and include/hrt_app.hpp's view_of / Context::reproject / next_frame_history (tests/cpp/history_demo) against
    the Python mirror's bytes on the box scene's geometry."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "history_demo.mk"], check=True)  # (up to date after build())
    _, settings = E.preset("box")
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
    r = subprocess.run([os.path.join(cpp, "history_demo"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    w, h = 48, 32
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [w, h] and len(raw) == 8 + w * h * (4 + 4 + 16)
    carried = np.frombuffer(raw[8:8 + w * h * 4], np.uint32).reshape(h, w)
    counts = np.frombuffer(raw[8 + w * h * 4:8 + w * h * 8], np.uint32).reshape(h, w)
    acc = np.frombuffer(raw[8 + w * h * 8:], F32).reshape(h, w, 4)
    # the demo's scene through the Python mirror: the same geometry, Lambertian grey, 1 sample, 4 bounces, light on
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    st = E.RayTracerSettings(num_samples=1, max_bounces=4, use_environment_lighting=True,
                             sphere_data=[E.Sphere(s.centre, s.radius, grey) for s in settings.sphere_data],
                             mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in settings.mesh_data])
    want = _demo_sequence(st, (w, h), _lib.MODE_RGBA32F)
    assert equal(carried, want[0]) and equal(counts, want[1]) and equal(acc, want[2])
