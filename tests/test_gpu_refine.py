"""Adaptive refinement on the device (hrt_refine_select, hrt_refine, hrt_refine_until): every bit
of the selection against the numpy restatement of S17 (tests/refine_ref.py), guided and not, at every radius; every
byte of the accumulator, the count image and the moments image after a refinement pass against a twin context that ran
hrt_trace + hrt_accumulate_history[_moments] (at the selected pixels) and against the state before (everywhere else),
by every method, in both context modes; then hrt_refine_until against the numpy chain, what the calls leave alone, the
rejections, and the Python and C++ mirrors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pyoracle
import refine_ref as R
import variance_ref as V
from helpers import E, SceneCase, _lib
from image_ref import same_floats
from test_gpu_history import CAP, DevBuf, synthetic_guide, synthetic_source

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xA5
TRACE, ACCUM = _lib.IMG_TRACE, _lib.IMG_ACCUM
RGBA8, RGBA32F = _lib.FMT_RGBA8, _lib.FMT_RGBA32F
MODES = [_lib.MODE_RGBA8, _lib.MODE_RGBA32F]
QUERIES, FRAME = _lib.REFINE_QUERIES, _lib.REFINE_FRAME
# (refinement method, query method): QUERIES by SCAN, BVH and PAIRS, AUTO, and FRAME
METHODS = [(QUERIES, _lib.QUERY_SCAN), (QUERIES, _lib.QUERY_BVH), (QUERIES, _lib.QUERY_PAIRS), (_lib.REFINE_AUTO, 0),
           (FRAME, 0)]
# 1x1 and 7x5: smaller than the window; 37x23: 851 pixels, a partial last word and a partial last wave; 64x64;
# 130x70: rows that straddle words and waves
SIZES = [(1, 1), (7, 5), (37, 23), (64, 64), (130, 70)]  # (width, height)
SCENES = {(1, 1): "box", (7, 5): "spheres", (37, 23): "box", (64, 64): "spheres", (130, 70): "box"}


def native(mode):
    return RGBA8 if mode == _lib.MODE_RGBA8 else RGBA32F


def equal(got, want):
    if want.dtype != F32:
        return got.tobytes() == want.tobytes()
    return got.shape == want.shape and bool(same_floats(got, want).all())


def report(got, want):
    same = same_floats(got, want) if want.dtype == F32 else got == want
    bad = np.argwhere(~same.reshape(same.shape[0], same.shape[1], -1).all(-1))
    y, x = bad[0]
    return f"{len(bad)} pixels differ; first at (x={x}, y={y}): {got[y, x]} vs {want[y, x]}"


def read_state(ctx, mode):
    return ctx.read(ACCUM, native(mode)), ctx.read_history(), ctx.read_moments()


def check_state(ctx, mode, want, what):
    for got, exp, name in zip(read_state(ctx, mode), want, ("accumulator", "counts", "moments")):
        assert equal(got, exp), (what, name, report(got, exp))


def masks_of(w, h, seed=4):
    """(name, selection) pairs: none, all, the first bit only, the last bit only, one whole word, alternate waves,
    random halves."""
    n = w * h
    i = np.arange(n)
    rng = np.random.default_rng([seed, w, h])
    word = (i >> 5) == min(1, (n - 1) >> 5)
    out = [("none", i < 0), ("all", i >= 0), ("first", i == 0), ("last", i == n - 1), ("word", word),
           ("alternate waves", ((i >> 6) & 1) == 0), ("half a", rng.uniform(size=n) < 0.5), ("half b", rng.uniform(size=n) < 0.5)]
    return [(name, m.reshape(h, w)) for name, m in out]


def mixed_history(ctx, case, mode, first_offset=1):
    """Counts 3..7 that differ inside every wave and the traced moments that go with them: three whole folds, then
    refinements over four striped masks (checked against the numpy chain here).  Returns the chain's (acc, cnt, mom)."""
    h, w = ctx.local_rows, ctx.width
    ctx.fill_history(0)
    acc = np.zeros((h, w, 4), np.uint8 if mode == _lib.MODE_RGBA8 else F32)
    cnt, mom = np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    off = first_offset
    for _ in range(3):
        ctx.trace(case.push(off))
        new = ctx.read(TRACE, native(mode))
        ctx.accumulate_history_moments(CAP)
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, CAP)
        off += 1
    i = np.arange(w * h).reshape(h, w)
    for k, sel in enumerate((i % 3 == 0, i % 7 < 3, i % 2 == 0, i % 5 == 0)):
        ctx.trace(case.push(off))
        new = ctx.read(TRACE, native(mode))
        ctx.refine(case.push(off), R.pack_mask(sel), CAP, FRAME if k & 1 else QUERIES)
        acc, cnt, mom = R.refine(acc, cnt, mom, new, sel, CAP, True)
        off += 1
    check_state(ctx, mode, (acc, cnt, mom), "mixed history")
    return acc, cnt, mom


# ---- 1. the selection ----------------------------------------------------------------------------------------------

def check_selection(ctx, cnt, mom, key, guide_ptr, rule, dev, what):
    want = R.select(cnt, mom, key, *rule)
    words = R.pack_mask(want)
    fields = dict(zip(("min_history", "max_count", "radius", "tolerance", "luminance_floor"), rule))
    mask, n = ctx.refine_select(guide_ptr, **fields)  # into host memory
    assert mask.tobytes() == words.tobytes(), (what, "host mask", int((R.unpack_mask(mask, cnt.shape) != want).sum()))
    assert n == int(want.sum()), (what, "selected", n, int(want.sum()))
    # into device memory: the same words, the bytes past the last word untouched
    assert dev.nbytes >= words.nbytes + 16
    ctx.refine_select_into(dev.ptr, guide_ptr, False, **fields)  # stream-ordered: no count, no wait
    ctx.synchronize()
    raw = dev.read()
    assert raw[:words.nbytes].tobytes() == words.tobytes(), (what, "device mask")
    assert (raw[words.nbytes:] == FILL).all(), (what, "past the end of the mask")
    assert ctx.refine_select_into(dev.ptr, guide_ptr, True, **fields) == n
    return want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_selection_bit_for_bit(size, mode):
    w, h = size
    case = SceneCase(SCENES[size], size, num_samples=1, max_bounces=2)
    ctx = case.context(mode=mode, debug=True)
    words = (w * h + 31) // 32
    dev = DevBuf(words * 4 + 64)
    d_real, d_synth = DevBuf(w * h * 32), DevBuf(w * h * 32)
    ctx.intersect_primary_into(case.push(), d_real.ptr)
    real = d_real.read().view(_lib.HIT_DTYPE).reshape(h, w)
    synth = synthetic_guide(w, h)
    d_synth.write(synth)
    guides = [(None, None), (R.keys_of(real, (h, w)), d_real.ptr), (R.keys_of(synth, (h, w)), d_synth.ptr)]
    # the first call allocates and zeroes N and M: every pixel is below min_history
    mask, n = ctx.refine_select()
    assert n == w * h and mask.tobytes() == R.pack_mask(np.ones((h, w), bool)).tobytes()
    # traced folds: per-pixel moments, counts 3..7 on both sides of min_history and max_count inside every wave
    _, cnt, mom = mixed_history(ctx, case, mode)
    if w * h >= 35:
        assert set(np.unique(cnt)) == {3, 4, 5, 6, 7}
    seen = []
    for key, ptr in guides:
        for radius in (0, 1, 3):
            for mh, mc, tol, fl in ((5, 7, 0.05, 0.01), (1, CAP, 0.3, 0.01), (4, 6, 1.0, 0.5), (3, 3, 0.05, 0.01)):
                sel = check_selection(ctx, cnt, mom, key, ptr, (mh, mc, radius, tol, fl), dev, (ptr is not None, radius, mh, mc, tol))
                seen.append(float(sel.mean()))
    if w * h >= 35:
        assert min(seen) < 1.0 and max(seen) > 0.0 and len(set(seen)) > 4  # the rules differ
    # uniform moments from hrt_fill_moments: NaN, infinities, m2 < m1^2; with the mixed counts and with uniform ones
    inf, nan = float("inf"), float("nan")
    for m1, m2 in ((nan, 1.0), (1.0, nan), (1.0, inf), (inf, inf), (-inf, 1.0), (1.0, 0.5), (0.5, 0.75), (0.0, 0.0)):
        ctx.fill_moments(m1, m2)
        um = np.empty((h, w, 2), F32)
        um[..., 0], um[..., 1] = m1, m2
        for key, ptr in guides[:2]:
            for radius in (0, 1, 3):
                check_selection(ctx, cnt, um, key, ptr, (4, 7, radius, 0.05, 0.01), dev, ("fill", m1, m2, radius))
    for count in (0, 3, 4, 2**32 - 1):
        ctx.fill_history(count)
        uc = np.full((h, w), count, np.uint32)
        check_selection(ctx, uc, um, None, None, (4, CAP, 1, 0.05, 0.01), dev, ("uniform count", count))
    assert ctx.check_guards()[1] == 0
    ctx.close()
    for b in (dev, d_real, d_synth):
        b.free()


# ---- 2. one refinement pass ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_refinement_against_a_twin_by_every_method(size, mode):
    w, h = size
    case = SceneCase(SCENES[size], size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, debug=True), case.context(mode=mode)
    src = synthetic_source(w, h, mode)
    pc = case.push(11)
    words = (w * h + 31) // 32
    dev = DevBuf(words * 4 + 64)
    cap = 8
    for count, (m1, m2) in ((0, (9.0, 9.0)), (3, (0.4, 0.9)), (8, (2.5, 0.125))):  # none, below the cap, at the cap
        before = (src, np.full((h, w), count, np.uint32), np.empty((h, w, 2), F32))
        before[2][..., 0], before[2][..., 1] = m1, m2

        def restore(c):
            c.load_accumulator(src)
            c.fill_history(count)
            c.fill_moments(m1, m2)

        restore(twin)
        twin.trace(pc)
        frame = twin.read(TRACE, native(mode))
        twin.accumulate_history_moments(cap)
        after = read_state(twin, mode)
        for name, sel in masks_of(w, h):
            want = tuple(np.where(sel.reshape(sel.shape + (1,) * (a.ndim - 2)), a, b) for a, b in zip(after, before))
            host = R.pack_mask(sel)
            if name == "last" and (w * h) % 32:  # bits of the last word beyond the image are ignored
                host[-1] |= np.uint32((0xFFFFFFFF << ((w * h) % 32)) & 0xFFFFFFFF)
            dev.write(host)
            for k, (method, qm) in enumerate(METHODS):
                restore(ctx)
                st = ctx.refine(pc, dev.ptr if k & 1 else host, cap, method, qm)
                check_state(ctx, mode, want, (count, name, method, qm))
                assert st.selected == int(sel.sum()) and st.reserved == 0
                if st.selected == 0:
                    assert (st.method_ran, st.query_method_ran, st.segments) == (0, 0, 0)
                elif method == FRAME or (method == _lib.REFINE_AUTO and st.method_ran == FRAME):
                    assert (st.method_ran, st.query_method_ran, st.segments) == (FRAME, 0, 0)
                    assert ctx.read(TRACE, native(mode)).tobytes() == frame.tobytes()  # exactly hrt_trace's image
                else:
                    assert st.method_ran == QUERIES and st.query_method_ran in (1, 2, 3)
                    assert qm in (0, _lib.QUERY_PAIRS) or st.query_method_ran == qm
            # without the moments flag M keeps every byte
            restore(ctx)
            ctx.refine(pc, host, cap, QUERIES, 0, moments=False)
            check_state(ctx, mode, (want[0], want[1], before[2]), (count, name, "no moments"))
        assert (dev.read()[words * 4:] == FILL).all()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    dev.free()


@pytest.mark.parametrize("mode", MODES)
def test_queries_leave_the_context_alone_and_count_the_oracles_segments(mode):
    size = w, h = (37, 23)
    for name in ("box", "spheres"):
        case = SceneCase(name, size, num_samples=1, max_bounces=2)
        ctx = case.context(mode=mode, debug=True, options={_lib.OPT_FOLD_RECORDS: 1})
        ctx.trace(case.push(1))
        ctx.accumulate_history_moments(CAP)
        ctx.trace(case.push(2))
        ctx.accumulate(1)
        target = DevBuf(w * h * 4)
        t0 = ctx.present(ACCUM, target.ptr, target.nbytes, w, h)
        trace = ctx.read(TRACE, native(mode))
        st0 = ctx.stats()
        stats = (st0.segments, st0.tri_tests, st0.traces, st0.accumulates, st0.last_kernel, st0.last_block, st0.last_frames)
        records = ctx.fold_records(with_total=True)
        sel = dict(masks_of(w, h))["half a"]
        ys, xs = np.nonzero(sel)
        pc = case.push(7)
        _, seg, tests = pyoracle.trace_pixels(pc, case.rays, case.spheres, case.tris, case.meshes, xs, ys)
        for qm in (_lib.QUERY_SCAN, _lib.QUERY_BVH, _lib.QUERY_PAIRS):
            st = ctx.refine(pc, R.pack_mask(sel), CAP, QUERIES, qm)
            assert (st.selected, st.segments, st.tri_tests) == (len(xs), seg, tests), (name, qm)
            assert st.scan_segments == 0
        assert ctx.read(TRACE, native(mode)).tobytes() == trace.tobytes()
        st1 = ctx.stats()
        assert (st1.segments, st1.tri_tests, st1.traces, st1.accumulates, st1.last_kernel, st1.last_block,
                st1.last_frames) == stats
        after = ctx.fold_records(with_total=True)
        assert after[1] == records[1] and after[0].tobytes() == records[0].tobytes()
        assert ctx.present(ACCUM, target.ptr, target.nbytes, w, h) == t0 + 1
        # FRAME counts in hrt_stats as hrt_trace does, and not as a fold
        ctx.refine(pc, R.pack_mask(sel), CAP, FRAME)
        st2 = ctx.stats()
        assert st2.traces == st1.traces + 1 and st2.accumulates == st1.accumulates and st2.segments > st1.segments
        assert ctx.check_guards()[1] == 0
        ctx.close()
        target.free()


# ---- 3. hrt_refine_until ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,size,method", [("box", (37, 23), QUERIES), ("spheres", (64, 64), FRAME),
                                              ("spheres", (130, 70), _lib.REFINE_AUTO)])
def test_refine_until_against_the_numpy_chain(name, size, method, mode):
    w, h = size
    case = SceneCase(name, size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, debug=True), case.context(mode=mode)
    d_hits = DevBuf(w * h * 32)
    ctx.intersect_primary_into(case.push(), d_hits.ptr)
    key = R.keys_of(d_hits.read().view(_lib.HIT_DTYPE), (h, w))
    acc, cnt, mom = mixed_history(ctx, case, mode)

    def frames(k):
        twin.trace(case.push(40 + k))
        return twin.read(TRACE, native(mode))

    rule = (5, 9, 1, 0.05, 0.01)
    want = R.refine_until(acc, cnt, mom, frames, CAP, 4, key, rule)
    got = ctx.refine_until(case.push(40), CAP, 4, d_hits.ptr, method, min_history=5, max_count=9, radius=1, tolerance=0.05,
                           luminance_floor=0.01)
    assert got == (want[3], want[4], want[5]) and want[3] == 4 and not want[5]
    assert len(set(want[6])) > 1 and want[6][-1] < w * h  # the selection shrinks: the passes differ
    check_state(ctx, mode, want[:3], "four passes")
    # a rule that selects nothing: settled at once, nothing changed
    got = ctx.refine_until(case.push(50), CAP, 4, d_hits.ptr, method, min_history=1, max_count=1)
    assert got == (0, 0, True)
    check_state(ctx, mode, want[:3], "settled")
    assert ctx.refine_until(case.push(50), CAP, 0, None, method) == (0, 0, False)
    # on into the per-pixel budget, unguided
    def later(k):
        twin.trace(case.push(60 + k))
        return twin.read(TRACE, native(mode))

    budget = R.refine_until(*want[:3], later, CAP, 8, None, (2, 9, 1, 1e-6, 0.01))
    got = ctx.refine_until(case.push(60), CAP, 8, None, method, min_history=2, max_count=9, tolerance=1e-6)
    assert got == (budget[3], budget[4], budget[5]) and budget[3] > 0
    check_state(ctx, mode, budget[:3], "the budget")
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    d_hits.free()


# ---- 4. what the new calls leave alone ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_the_old_entry_points_give_the_same_bytes_before_and_after(mode):
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, debug=True), case.context(mode=mode)
    d_hits = DevBuf(w * h * 32)
    ctx.intersect_primary_into(case.push(), d_hits.ptr)

    def old_calls(c, first):
        for k in range(3):
            c.trace(case.push(first + k))
            c.accumulate_history_moments(16)
        out = [read_state(c, mode), c.denoise_variance(RGBA32F, d_hits.ptr, with_variance=True)]
        saved = c.read(ACCUM, native(mode))
        c.compute_n(case.push(first + 10), 3)
        out.append(c.read(ACCUM, native(mode)))
        c.load_accumulator(saved)
        return out

    def same(a, b):
        flat = lambda t: [x for y in t for x in (y if isinstance(y, tuple) else (y,))]  # noqa: E731
        return all(x.tobytes() == y.tobytes() for x, y in zip(flat(a), flat(b)))

    assert same(old_calls(ctx, 1), old_calls(twin, 1))
    # the new calls on ctx; the twin follows with the plain calls (a refinement of every pixel is the history fold)
    mask, n = ctx.refine_select(d_hits.ptr)
    assert 0 < n <= w * h
    everything = R.pack_mask(np.ones((h, w), bool))
    for k, method in enumerate((QUERIES, FRAME)):
        ctx.refine(case.push(30 + k), everything, 16, method)
        twin.trace(case.push(30 + k))
        twin.accumulate_history_moments(16)
    ctx.refine_until(case.push(90), 16, 2, d_hits.ptr, min_history=1, max_count=1)
    assert same(read_state(ctx, mode), read_state(twin, mode))
    assert same(old_calls(ctx, 50), old_calls(twin, 50))
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    d_hits.free()


# ---- 5. the rejections -------------------------------------------------------------------------------------------------

def test_rejections_enqueue_nothing_and_leave_the_context_usable():
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context()
    ctx.trace(case.push(1))
    ctx.accumulate_history_moments(4)
    lib, handle = ctx.lib, ctx.handle
    words = (w * h + 31) // 32
    d_hits, d_mask = DevBuf(w * h * 32 + 16), DevBuf(words * 4 + 16)
    ctx.intersect_primary_into(case.push(), d_hits.ptr)
    state, st0 = read_state(ctx, ctx.mode), ctx.stats()
    host_raw = np.zeros(w * h * 32 + 16, np.uint8)
    host_hits = host_raw.ctypes.data + (-host_raw.ctypes.data) % 16  # aligned, but pageable host memory
    mask = np.full(words, 0xFFFFFFFF, np.uint32)
    n, stats = ctypes.c_uint64(5), _lib.RefineStats()
    passes, frames, settled = ctypes.c_uint32(5), ctypes.c_uint64(5), ctypes.c_uint32(5)
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    err = lambda: lib.hrt_last_error(handle)  # noqa: E731

    out_mask = np.zeros(words, np.uint32)

    def select(rule=ctx.refine_rule(), guide=d_hits.ptr, m=out_mask.ctypes.data):
        return lib.hrt_refine_select(handle, ref(rule), ctypes.c_void_p(guide or 0), ctypes.c_void_p(m or 0), ctypes.byref(n))

    def refine(pc=case.push(5), m=mask.ctypes.data, max_history=8, method=0, qm=0, flags=1):
        return lib.hrt_refine(handle, ref(pc), ctypes.c_void_p(m or 0), max_history, method, qm, flags, ctypes.byref(stats))

    def until(pc=case.push(5), rule=ctx.refine_rule(), guide=d_hits.ptr, max_history=8, method=0, flags=0, out=passes,
              out2=frames):
        return lib.hrt_refine_until(handle, ref(pc), ref(rule), ctypes.c_void_p(guide or 0), max_history, 4, method, flags,
                                    ref(out), ref(out2), ctypes.byref(settled))

    assert select(rule=None) == 1 and b"null" in err()
    assert select(m=None) == 1 and b"null" in err()
    assert refine(pc=None) == 1 and b"null" in err()
    assert refine(m=None) == 1 and b"null" in err()
    assert until(pc=None) == 1 and b"null" in err()
    assert until(rule=None) == 1 and b"null" in err()
    assert until(out=None) == 1 and b"null" in err()
    assert until(out2=None) == 1 and b"null" in err()
    for fields, word in ((dict(flags=1), b"flags"), (dict(min_history=0), b"min_history"),
                         (dict(min_history=5, max_count=4), b"max_count"), (dict(radius=4), b"radius"),
                         (dict(tolerance=0.0), b"tolerance"), (dict(tolerance=float("nan")), b"tolerance"),
                         (dict(tolerance=float("inf")), b"tolerance"), (dict(tolerance=-0.1), b"tolerance"),
                         (dict(luminance_floor=0.0), b"luminance_floor"), (dict(luminance_floor=float("nan")), b"luminance_floor"),
                         (dict(luminance_floor=float("inf")), b"luminance_floor")):
        rule = ctx.refine_rule()
        for k, v in fields.items():
            setattr(rule, k, v)
        assert select(rule=rule) == 1 and word in err(), fields
        assert until(rule=rule) == 1 and word in err(), fields
    assert select(guide=host_hits) == 1 and b"device" in err()
    assert select(guide=d_hits.ptr + 8) == 1 and b"aligned" in err()
    assert select(m=d_mask.ptr + 2) == 1 and b"aligned" in err()
    assert until(guide=host_hits) == 1 and b"device" in err()
    assert until(guide=d_hits.ptr + 8) == 1 and b"aligned" in err()
    assert refine(m=d_mask.ptr + 2) == 1 and b"aligned" in err()
    assert refine(method=3) == 1 and b"unknown method" in err()
    assert until(method=3) == 1 and b"unknown method" in err()
    assert refine(qm=4) == 1 and b"query method" in err()
    assert refine(flags=2) == 1 and b"flag" in err()
    assert until(flags=2) == 1 and b"flag" in err()
    for bad in (0, CAP + 1, 2**32 - 1):
        assert refine(max_history=bad) == 1 and b"max_history" in err()
        assert until(max_history=bad) == 1 and b"max_history" in err()
    for change, word in ((dict(init=1), b"init"), (dict(width=w + 1), b"width"), (dict(height=h - 1), b"width"),
                         (dict(num_spheres=99), b"exceed"), (dict(num_meshes=99), b"exceed"), (dict(num_meshes=-1), b"exceed")):
        pc = case.push(5)
        for k, v in change.items():
            setattr(pc, k, v)
        assert refine(pc=pc) == 1 and word in err(), change
        assert until(pc=pc) == 1 and word in err(), change
    # nothing was enqueued or written: the state, the statistics and the outputs are as they were
    assert all(a.tobytes() == b.tobytes() for a, b in zip(read_state(ctx, ctx.mode), state))
    st1 = ctx.stats()
    assert (st1.traces, st1.accumulates, st1.segments) == (st0.traces, st0.accumulates, st0.segments)
    assert (n.value, passes.value, frames.value, settled.value) == (5, 5, 5, 5) and (d_mask.read() == FILL).all()
    assert (out_mask == 0).all() and (mask == 0xFFFFFFFF).all()
    # the edges of the accepted ranges, and the calls still work
    edge = ctx.refine_rule(min_history=1, max_count=1, radius=3, tolerance=1e-30, luminance_floor=1e-30)
    assert select(rule=edge) == 0 and n.value == 0
    assert refine(max_history=CAP, method=2, qm=3) == 0 and stats.selected == w * h
    assert until() == 0
    ctx.close()
    # no scene
    bare = E.HrtContext(size, device=0)
    with pytest.raises(_lib.HrtError, match="HRT_ERR_NO_SCENE"):
        bare.refine(case.push(5), mask, 8)
    with pytest.raises(_lib.HrtError, match="HRT_ERR_NO_SCENE"):
        bare.refine_until(case.push(5), 8, 2)
    assert bare.refine_select()[1] == w * h  # the selection needs no scene
    bare.close()
    # a row-tile partition, with and without a communicator, and an unpartitioned context joined to one
    parts = [case.context(partition=(8, p, 2)) for p in range(2)]
    for joined in (False, True):
        if joined:
            E.HrtContext.comm_init_all(parts)
        for c in parts:
            for call in (c.refine_select, lambda: c.refine(case.push(5), mask, 8),
                         lambda: c.refine_until(case.push(5), 8, 2)):
                with pytest.raises(_lib.HrtError, match="partition"):
                    call()
    for c in parts:
        c.close()
    single = case.context()
    E.HrtContext.comm_init_all([single])
    for call in (single.refine_select, lambda: single.refine(case.push(5), mask, 8),
                 lambda: single.refine_until(case.push(5), 8, 2)):
        with pytest.raises(_lib.HrtError, match="communicator"):
            call()
    single.close()
    d_hits.free()
    d_mask.free()


# ---- 6. the mirrors ----------------------------------------------------------------------------------------------------

def _demo_sequence(settings, size):
    """What tests/cpp/refine_demo.cpp does, through the Python mirror: four history frames with moments, the
    selection under the defaults guided by the first hits, then hrt_refine_until for three passes.  Returns (mask,
    selected, passes, pixel_frames, counts, accumulator), checked here against the numpy chain."""
    w, h = size
    ctx = E.HrtContext(size, device=0, mode=_lib.MODE_RGBA32F)
    twin = E.HrtContext(size, device=0, mode=_lib.MODE_RGBA32F)
    pipe, diffuse = E.RayTracePipeline(ctx, size, settings), E.DiffusePipeline(ctx, size)
    tpipe = E.RayTracePipeline(twin, size, settings)
    cam = E.Camera([3.0, 1.5, 2.0], [-0.8, -0.3, -0.6])  # outside the box: noisy walls, a settled sky
    acc, cnt, mom = np.zeros((h, w, 4), F32), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    for frame in range(4):
        pipe.compute(cam, frame)
        diffuse.next_frame_history(pipe.image(), 1 << 24, moments=True)
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, ctx.read(TRACE, RGBA32F), 1 << 24)
    d_hits = DevBuf(w * h * 32)
    pipe.first_hits_async(cam, d_hits.ptr)
    mask, n = ctx.refine_select(d_hits.ptr)
    key = R.keys_of(d_hits.read().view(_lib.HIT_DTYPE), (h, w))
    assert mask.tobytes() == R.pack_mask(R.select(cnt, mom, key)).tobytes() and 0 < n < w * h

    def frames(k):
        tpipe.compute(cam, 4 + k)
        return twin.read(TRACE, RGBA32F)

    want = R.refine_until(acc, cnt, mom, frames, 1 << 24, 3, key)
    passes, pixel_frames, settled = diffuse.refine_until(pipe, cam, 4, 3, guide_ptr=d_hits.ptr)
    assert (passes, pixel_frames, settled) == (want[3], want[4], want[5]) and passes == 3
    out = mask, n, passes, pixel_frames, ctx.read_history(), ctx.read(ACCUM, RGBA32F)
    assert equal(out[4], want[1]) and equal(out[5], want[0]), report(out[5], want[0])
    ctx.close()
    twin.close()
    d_hits.free()
    return out


def test_python_and_cpp_mirrors(tmp_path):
    """HrtContext.refine_select / refine_until and DiffusePipeline.refine_until against the numpy chain, and
    include/hrt_app.hpp's Context::refine_select / refine / refine_until and DiffusePipeline::refine_until
    (tests/cpp/refine_demo) against the Python mirror's bytes on the box scene's geometry."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "refine_demo.mk"], check=True)  # (up to date after build())
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
    r = subprocess.run([os.path.join(cpp, "refine_demo"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    w, h = 48, 32
    words = (w * h + 31) // 32
    head = np.frombuffer(raw[:32], np.uint64)
    assert head[:2].tolist() == [w, h] and len(raw) == 32 + words * 4 + w * h * (4 + 16)
    mask = np.frombuffer(raw[32:32 + words * 4], np.uint32)
    counts = np.frombuffer(raw[32 + words * 4:32 + words * 4 + w * h * 4], np.uint32).reshape(h, w)
    acc = np.frombuffer(raw[32 + words * 4 + w * h * 4:], F32).reshape(h, w, 4)
    # the demo's scene through the Python mirror: the same geometry, Lambertian grey, 1 sample, 4 bounces, light on
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    st = E.RayTracerSettings(num_samples=1, max_bounces=4, use_environment_lighting=True,
                             sphere_data=[E.Sphere(s.centre, s.radius, grey) for s in settings.sphere_data],
                             mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in settings.mesh_data])
    want = _demo_sequence(st, (w, h))
    assert mask.tobytes() == want[0].tobytes()
    assert int(head[2]) == want[1] and int(head[3]) == want[3]  # selected by the first call; pixel-frames of the three passes
    assert equal(counts, want[4]) and equal(acc, want[5]), report(acc, want[5])
