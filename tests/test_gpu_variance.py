"""The variance-guided denoise on the device (hrt_accumulate_history_moments, hrt_reproject_moments, hrt_fill_moments,
hrt_read_moments, hrt_denoise_variance, hrt_denoise_variance_present): every byte of the
accumulator, the count image, the moments image, the filtered image and the filtered variance against the numpy
restatement of S16 (tests/variance_ref.py), NaN compared as NaN, in both context modes.  The accumulator and the
count image are also held to a twin context that runs the plain history calls.  Accumulators are loaded (bytes;
floats above 1, NaN and infinite texels), moments come from hrt_fill_moments (NaN and infinities among them) and
from folds of traced frames, mixed counts from the rejections of reprojections; trace texels are traced frames and,
through a scene of lights with chosen emissions, every byte and the adversarial floats (above 1, NaN, infinities);
guides are synthetic or the real first hits of box and spheres on either side of a real camera move.  Then what
the calls leave alone, the rejections, and the Python and C++ mirrors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import history_ref as H
import present_ref
import variance_ref as V
from helpers import E, SceneCase, _lib
from image_ref import same_floats
from test_gpu_history import CAP, DevBuf, hip, synthetic_guide, synthetic_source, turned, view_pairs
from test_gpu_image_exhaustive import Columns, byte_case, float_emissions

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xA5
TRACE, ACCUM = _lib.IMG_TRACE, _lib.IMG_ACCUM
RGBA8, RGBA32F = _lib.FMT_RGBA8, _lib.FMT_RGBA32F
MODES = [_lib.MODE_RGBA8, _lib.MODE_RGBA32F]
FILTERS = [_lib.REPROJECT_NEAREST, _lib.REPROJECT_BILINEAR]
METHODS = [_lib.VARIANCE_AUTO, _lib.VARIANCE_DIRECT, _lib.VARIANCE_TILED]
# 1x1, 2x2; 7x5: smaller than the 7x7 window and than the 5x5 window at step 2; 37x23: wider than one 32-wide tile,
# the step-16 taps leave the image on every side; 64x64; 130x70: several tiles in both axes
SIZES = [(1, 1), (2, 2), (7, 5), (37, 23), (64, 64), (130, 70)]  # (width, height)


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


def refill(buf):
    assert hip().hipMemset(buf.ptr, FILL, buf.nbytes) == 0 and hip().hipDeviceSynchronize() == 0


def check_state(ctx, mode, acc, cnt, mom, what, twin=None):
    got = ctx.read(ACCUM, native(mode))
    assert equal(got, acc), (what, "accumulator", report(got, acc))
    got_n = ctx.read_history()
    assert equal(got_n, cnt), (what, "counts", report(got_n, cnt))
    got_m = ctx.read_moments()
    assert equal(got_m, mom), (what, "moments", report(got_m, mom))
    if twin is not None:  # the plain history calls on a twin context: the same bytes in A and N
        assert twin.read(ACCUM, native(mode)).tobytes() == got.tobytes(), (what, "twin accumulator")
        assert twin.read_history().tobytes() == got_n.tobytes(), (what, "twin counts")


def traced_moments(ctx, case, offsets):
    """Moments that differ from pixel to pixel: the context's history restarted and the frames of `offsets` folded.
    Returns the numpy chain's (acc, cnt, mom) of the same."""
    ctx.fill_history(0)
    mode = ctx.mode
    h, w = ctx.local_rows, ctx.width
    acc = np.zeros((h, w, 4), np.uint8 if mode == _lib.MODE_RGBA8 else F32)
    cnt, mom = np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    for off in offsets:
        ctx.trace(case.push(off))
        new = ctx.read(TRACE, native(mode))
        ctx.accumulate_history_moments(CAP)
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, CAP)
    return acc, cnt, mom


# ---- 1. the moments fold -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_moments_fold_with_per_pixel_counts(size, mode):
    w, h = size
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, debug=True), case.context(mode=mode)
    for c in (ctx, twin):
        c.trace(case.push(1))
    new = ctx.read(TRACE, native(mode))
    assert twin.read(TRACE, native(mode)).tobytes() == new.tobytes()
    src = synthetic_source(w, h, mode)
    assert (ctx.read_moments().view(np.uint32) == 0).all()  # allocated and zeroed by the first call
    # uniform counts: none, one, below / at / above the cap, the largest cap, and the count whose successor wraps;
    # uniform moments, NaN and infinities among them, then the per-pixel moments the first fold leaves
    fills = [(0.37, 1.9), (0.0, 0.0), (float("nan"), float("inf")), (float("-inf"), -0.0), (3.5, 0.25)]
    for k, (count, cap) in enumerate(((0, 32), (1, 32), (31, 32), (32, 32), (40, 32), (CAP - 1, CAP), (CAP, CAP),
                                      (2**32 - 1, CAP), (5, 1))):
        m1, m2 = fills[k % len(fills)]
        for c in (ctx, twin):
            c.load_accumulator(src)
            c.fill_history(count)
        ctx.fill_moments(m1, m2)
        acc, cnt = src, np.full((h, w), count, np.uint32)
        mom = np.empty((h, w, 2), F32)
        mom[..., 0], mom[..., 1] = m1, m2
        check_state(ctx, mode, acc, cnt, mom, ("fill", count))
        for rep in range(2):
            ctx.accumulate_history_moments(cap)
            twin.accumulate_history(cap)
            acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, cap)
            check_state(ctx, mode, acc, cnt, mom, ("fold", count, cap, rep), twin)
    # mixed counts: what a reprojection with rejections leaves, folded twice
    hits = synthetic_guide(w, h)
    other = hits.copy()
    other["kind"][::2, 1::3] = 0
    d_prev, d_cur = DevBuf(w * h * 32).write(other), DevBuf(w * h * 32).write(hits)
    view = view_pairs(size)[0][1]
    for c in (ctx, twin):
        c.load_accumulator(src)
        c.fill_history(6)
    ctx.reproject_moments(view, d_prev.ptr, view, d_cur.ptr, filter=_lib.REPROJECT_NEAREST, depth_tolerance=0.5)
    twin.reproject(view, d_prev.ptr, view, d_cur.ptr, filter=_lib.REPROJECT_NEAREST, depth_tolerance=0.5)
    acc, cnt, mom = V.reproject_moments(src, np.full((h, w), 6, np.uint32), mom, view.record, other, view.record, hits,
                                        H.NEAREST, 0.5)
    check_state(ctx, mode, acc, cnt, mom, "mixed", twin)
    if w * h >= 15:
        assert set(np.unique(cnt)) == {0, 6}
    for cap in (32, 7):
        for c in (ctx, twin):
            c.trace(case.push(2 + cap))
        new = ctx.read(TRACE, native(mode))
        ctx.accumulate_history_moments(cap)
        twin.accumulate_history(cap)
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, cap)
        check_state(ctx, mode, acc, cnt, mom, ("mixed fold", cap), twin)
    buffers, corrupted = ctx.check_guards()
    assert buffers > 0 and corrupted == 0
    ctx.close()
    twin.close()
    d_prev.free()
    d_cur.free()


@pytest.mark.parametrize("mode", MODES)
def test_moments_fold_of_chosen_trace_texels(mode):
    """Trace texels chosen through the emissions of tests/test_gpu_image_exhaustive.py's sphere scene (column j of
    the trace image shows light j): every byte value in RGBA8 mode; in RGBA32F mode the adversarial float pool --
    floats above 1, FLT_MAX, denormals, NaN and infinities."""
    size = w, h = (256, 5)
    case = byte_case(size) if mode == _lib.MODE_RGBA8 else Columns(size, float_emissions())
    ctx, twin = case.context(mode=mode, debug=True), case.context(mode=mode)
    for c in (ctx, twin):
        c.trace(case.push(1))
    new = ctx.read(TRACE, native(mode))
    if mode == _lib.MODE_RGBA8:
        assert len(np.unique(new[..., 0])) == 256
    else:
        rgb = new[..., :3]
        assert np.isnan(rgb).any() and np.isinf(rgb).any()
        assert (rgb[np.isfinite(rgb)] > 1).any()
    src = synthetic_source(w, h, mode)
    for count, (m1, m2) in ((0, (9.0, 9.0)), (1, (0.3, 0.7)), (7, (2.5, 0.125)), (2**32 - 1, (1.0, 1.0))):
        for c in (ctx, twin):
            c.load_accumulator(src)
            c.fill_history(count)
        ctx.fill_moments(m1, m2)
        acc, cnt = src, np.full((h, w), count, np.uint32)
        mom = np.empty((h, w, 2), F32)
        mom[..., 0], mom[..., 1] = m1, m2
        for rep in range(2):
            ctx.accumulate_history_moments(32)
            twin.accumulate_history(32)
            acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, 32)
            check_state(ctx, mode, acc, cnt, mom, ("chosen texels", count, rep), twin)
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()


# ---- 2. the moments reprojection over synthetic accumulators, counts and guides ---------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_moments_reprojection_of_synthetic_history(size, mode):
    w, h = size
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, debug=True), case.context(mode=mode)
    src = synthetic_source(w, h, mode)
    prev_hits, cur_hits = synthetic_guide(w, h, seed=2), synthetic_guide(w, h, seed=2)
    rng = np.random.default_rng([7, w, h])
    change = rng.uniform(size=(h, w)) < 0.15  # the previous view saw another surface, depth or normal there
    prev_hits["mesh"][change & (prev_hits["kind"] == 2)] += 1
    with np.errstate(over="ignore"):  # (a FLT_MAX depth becomes an infinity: one more edge value)
        prev_hits["t"][change & (prev_hits["kind"] == 1)] *= F32(1.01)
    d_prev, d_cur = DevBuf(w * h * 32).write(prev_hits), DevBuf(w * h * 32).write(cur_hits)
    guarded = None
    for name, prev, cur in view_pairs(size):
        for filt in FILTERS:
            for tol, mind in (H.DEFAULTS, (1e30, -2.0)):
                count = CAP if filt == _lib.REPROJECT_NEAREST else 9
                _, _, mom = traced_moments(ctx, case, (3, 4))  # per-pixel moments, m2 above m1^2 in places
                if w * h >= 15:
                    assert len(np.unique(mom[..., 0])) > 4
                for c in (ctx, twin):
                    c.load_accumulator(src)
                    c.fill_history(count)
                acc, cnt = src, np.full((h, w), count, np.uint32)
                for rep in range(2):
                    ctx.reproject_moments(prev, d_prev.ptr, cur, d_cur.ptr, filter=filt, depth_tolerance=tol, min_normal_dot=mind)
                    twin.reproject(prev, d_prev.ptr, cur, d_cur.ptr, filter=filt, depth_tolerance=tol, min_normal_dot=mind)
                    acc, cnt, mom = V.reproject_moments(acc, cnt, mom, prev.record, prev_hits, cur.record, cur_hits, filt,
                                                        tol, mind)
                    check_state(ctx, mode, acc, cnt, mom, (name, filt, tol, mind, rep), twin)
                    assert (mom[cnt == 0].view(np.uint32) == 0).all()  # a rejected pixel's moments are (0, 0)
                    if rep == 0:
                        for c in (ctx, twin):
                            c.trace(case.push(5))
                        new = ctx.read(TRACE, native(mode))
                        ctx.accumulate_history_moments(CAP)
                        twin.accumulate_history(CAP)
                        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, CAP)
                        check_state(ctx, mode, acc, cnt, mom, (name, filt, tol, mind, "fold"), twin)
                if name == "zero dx":
                    assert (cnt == 0).all()
                now = ctx.check_guards()
                assert now[1] == 0 and (guarded is None or now[0] == guarded)  # the buffers are reused
                guarded = now[0]
    assert d_prev.read().tobytes() == prev_hits.tobytes() and d_cur.read().tobytes() == cur_hits.tobytes()
    ctx.close()
    twin.close()
    d_prev.free()
    d_cur.free()


# ---- 3. the filter ------------------------------------------------------------------------------------------------------

def check_filter(ctx, acc, cnt, mom, hits, guide_ptr, fields, params, bufs):
    """One configuration against the reference: both formats, host and device destinations, with and without the
    variance."""
    dev32, dev8, devv = bufs
    iterations = fields["iterations"]
    want32, wantv = V.denoise_variance(acc, cnt, mom, iterations, params, hits)
    want8, _ = V.denoise_variance(acc, cnt, mom, iterations, params, hits, fmt_rgba8=True)
    for method in METHODS:
        f = dict(fields, method=method)
        for fmt, want, dev in ((RGBA32F, want32, dev32), (RGBA8, want8, dev8)):
            got = ctx.denoise_variance(fmt, guide_ptr, **f)
            assert equal(got, want), (f, fmt, "host, no variance", report(got, want))
            got, var = ctx.denoise_variance(fmt, guide_ptr, with_variance=True, **f)
            assert equal(got, want), (f, fmt, "host", report(got, want))
            assert equal(var, wantv), (f, fmt, "host variance", report(var, wantv))
            refill(dev)
            refill(devv)
            ctx.denoise_variance_into(dev.ptr, want.nbytes, fmt, guide_ptr, devv.ptr, wantv.nbytes, **f)
            raw, rawv = dev.read(), devv.read()
            got = raw[:want.nbytes].view(want.dtype).reshape(want.shape)
            var = rawv[:wantv.nbytes].view(F32).reshape(wantv.shape)
            assert equal(got, want), (f, fmt, "device", report(got, want))
            assert equal(var, wantv), (f, fmt, "device variance", report(var, wantv))
            assert (raw[want.nbytes:] == FILL).all() and (rawv[wantv.nbytes:] == FILL).all(), (f, fmt)
            refill(dev)
            ctx.denoise_variance_into(dev.ptr, want.nbytes, fmt, guide_ptr, **f)  # device image, no variance
            raw = dev.read()
            assert equal(raw[:want.nbytes].view(want.dtype).reshape(want.shape), want), (f, fmt, "device, no variance")
            assert (raw[want.nbytes:] == FILL).all()
    return want32, wantv


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_filter_of_synthetic_accumulators_moments_and_counts(size, mode):
    w, h = size
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context(mode=mode, debug=True)
    src = synthetic_source(w, h, mode)
    hits = synthetic_guide(w, h)
    d_guide = DevBuf(w * h * 32).write(hits)
    # moments of two traced frames; then counts {0, 6} scattered inside every wave and tile (a reprojection through the
    # identity view whose previous guide misses at every third column of every other row), one more fold: {1, 7}
    _, _, mom = traced_moments(ctx, case, (3, 4))
    other = hits.copy()
    other["kind"][::2, 1::3] = 0
    d_prev = DevBuf(w * h * 32).write(other)
    view = view_pairs(size)[0][1]
    ctx.fill_history(6)
    ctx.reproject_moments(view, d_prev.ptr, view, d_guide.ptr, filter=_lib.REPROJECT_NEAREST, depth_tolerance=0.5)
    # (the accumulator is loaded below: only the counts and the moments of the chain are kept)
    acc, cnt, mom = V.reproject_moments(src, np.full((h, w), 6, np.uint32), mom, view.record, other, view.record, hits,
                                        H.NEAREST, 0.5)
    ctx.trace(case.push(5))
    new = ctx.read(TRACE, native(mode))
    ctx.accumulate_history_moments(32)
    _, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, 32)
    ctx.load_accumulator(src)  # (leaves the counts and the moments alone)
    check_state(ctx, mode, src, cnt, mom, "inputs")
    if w * h >= 15:
        assert set(np.unique(cnt)) == {1, 7}
    bufs = (DevBuf(w * h * 16 + 64), DevBuf(w * h * 4 + 64), DevBuf(w * h * 4 + 64))
    for guide, guide_ptr in ((None, None), (hits, d_guide.ptr)):
        for iterations in (0, 1, 3, 5):
            _, v = check_filter(ctx, src, cnt, mom, guide, guide_ptr, dict(iterations=iterations), V.DEFAULTS, bufs)
        if guide is None and w * h >= 15 and mode == _lib.MODE_RGBA8:
            assert np.isfinite(v).all() and (v > 0).any()  # (finite inputs, every centre tap has weight 1)
    # the threshold between the two estimates: every pixel temporal, the mix, every pixel spatial; other parameters
    for min_history in (1, 7, 8):
        check_filter(ctx, src, cnt, mom, hits, d_guide.ptr, dict(iterations=2, min_history=min_history),
                     V.DEFAULTS[:2] + (min_history,) + V.DEFAULTS[3:], bufs)
    odd = (0.7, 1e-4, 7, 1.5, 0.02)
    check_filter(ctx, src, cnt, mom, hits, d_guide.ptr,
                 dict(iterations=5, sigma_variance=odd[0], variance_floor=odd[1], min_history=odd[2], sigma_normal=odd[3],
                      sigma_depth=odd[4]), odd, bufs)
    # the filter wrote none of its inputs
    check_state(ctx, mode, src, cnt, mom, "after")
    assert d_guide.read().tobytes() == hits.tobytes()
    buffers, corrupted = ctx.check_guards()
    assert buffers > 0 and corrupted == 0
    ctx.close()
    for b in (d_guide, d_prev) + bufs:
        b.free()


def _stats_tuple(st):
    # (timings and wave_steps depend on scheduling: tests/test_gpu_intersect.py)
    return (st.segments, st.tri_tests, st.traces, st.last_kernel, st.last_block, st.last_frames)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["box", "spheres"])
def test_four_frame_chain_across_real_moves(name, mode):
    size = w, h = (64, 64)
    case = SceneCase(name, size, num_samples=1, max_bounces=4)
    ctx = case.context(mode=mode, debug=True, options={_lib.OPT_FOLD_RECORDS: 1})
    twin = case.context(mode=mode)
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
    cnt, mom = np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    hits = view = None
    for k, cam in enumerate(cams):
        case.camera = cam
        cur_view = E.View(cam, size, case.settings)
        ctx.intersect_primary_into(case.push(), d_hits[k & 1].ptr)
        cur_hits = d_hits[k & 1].read().view(_lib.HIT_DTYPE).reshape(h, w)
        for c in (ctx, twin):
            c.trace(case.push(1 + k))
        new = ctx.read(TRACE, native(mode))
        stats, accumulates = _stats_tuple(ctx.stats()), ctx.stats().accumulates
        if k:
            filt = FILTERS[k & 1]
            ctx.reproject_moments(view, d_hits[(k - 1) & 1].ptr, cur_view, d_hits[k & 1].ptr, filter=filt)
            twin.reproject(view, d_hits[(k - 1) & 1].ptr, cur_view, d_hits[k & 1].ptr, filter=filt)
            acc, cnt, mom = V.reproject_moments(acc, cnt, mom, view.record, hits, cur_view.record, cur_hits, filt, *H.DEFAULTS)
            check_state(ctx, mode, acc, cnt, mom, (k, "reproject"), twin)
            assert 0.5 < float((cnt > 0).mean()) < 1.0  # the move carries most of the history, not all of it
            assert ctx.stats().accumulates == accumulates
        ctx.accumulate_history_moments(32)
        twin.accumulate_history(32)
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, new, 32)
        check_state(ctx, mode, acc, cnt, mom, (k, "fold"), twin)
        # the trace image, the hit arrays and everything in hrt_stats but `accumulates` are as they were
        assert ctx.read(TRACE, native(mode)).tobytes() == new.tobytes()
        assert d_hits[k & 1].read().tobytes() == cur_hits.tobytes()
        assert _stats_tuple(ctx.stats()) == stats and ctx.stats().accumulates == accumulates + 1
        hits, view = cur_hits, cur_view
    assert set(np.unique(cnt)) <= {1, 2, 3, 4} and len(np.unique(cnt)) >= 3  # counts on both sides of min_history
    # the last stage: the variance-guided filter over the history, guided by the current first hits
    stats, accumulates = _stats_tuple(ctx.stats()), ctx.stats().accumulates
    bufs = (DevBuf(w * h * 16 + 64), DevBuf(w * h * 4 + 64), DevBuf(w * h * 4 + 64))
    last = d_hits[(len(cams) - 1) & 1].ptr
    for iterations in (0, 1, 3, 5):
        check_filter(ctx, acc, cnt, mom, hits, last, dict(iterations=iterations), V.DEFAULTS, bufs)
    check_filter(ctx, acc, cnt, mom, None, None, dict(iterations=5), V.DEFAULTS, bufs)
    check_state(ctx, mode, acc, cnt, mom, "after the filter", twin)
    assert ctx.read(TRACE, native(mode)).tobytes() == new.tobytes()
    assert _stats_tuple(ctx.stats()) == stats and ctx.stats().accumulates == accumulates
    # no fold record was appended, no ticket issued
    after = ctx.fold_records(with_total=True)
    assert after[1] == records[1] and after[0].tobytes() == records[0].tobytes()
    assert ctx.present(ACCUM, target.ptr, target.nbytes, w, h) == t0 + 1
    # hrt_denoise on the same accumulator: the twin's bytes
    assert ctx.denoise(RGBA32F, last).tobytes() == twin.denoise(RGBA32F, last).tobytes()
    ctx.synchronize()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    for b in d_hits + [target] + list(bufs):
        b.free()


# ---- 4. hrt_denoise_variance_present -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_denoise_variance_present(mode):
    size = w, h = (64, 36)
    case = SceneCase("box", size, num_samples=1, max_bounces=4)
    ctx = case.context(mode=mode, debug=True)
    acc, cnt, mom = traced_moments(ctx, case, (1, 2, 3))
    d_guide = DevBuf(w * h * 32)
    ctx.intersect_primary_into(case.push(), d_guide.ptr)
    hits = d_guide.read().view(_lib.HIT_DTYPE).reshape(h, w)
    plain = DevBuf(w * h * 4)
    t0 = ctx.present(ACCUM, plain.ptr, plain.nbytes, w, h)
    shots = [  # target size, pitch padding, offset, byte order, guide, method, iterations
        ((w, h), 0, 0, _lib.PRESENT_B8G8R8A8, True, _lib.VARIANCE_AUTO, 5),
        ((w, h), 20, 16, _lib.PRESENT_R8G8B8A8, True, _lib.VARIANCE_TILED, 5),
        ((w, h), 4, 4, _lib.PRESENT_B8G8R8A8, False, _lib.VARIANCE_DIRECT, 3),
        ((50, 31), 12, 0, _lib.PRESENT_R8G8B8A8, True, _lib.VARIANCE_TILED, 0),
        ((97, 80), 0, 8, _lib.PRESENT_B8G8R8A8, True, _lib.VARIANCE_AUTO, 1),
    ]
    targets, tickets = [], []
    for (wt, ht), pad, offset, order, guided, method, iterations in shots:
        pitch = wt * 4 + pad
        buf = DevBuf(offset + ht * pitch + 256)
        tickets.append(ctx.denoise_variance_present(buf.ptr + offset, ht * pitch, wt, ht, pitch, order,
                                                    d_guide.ptr if guided else None, method=method, iterations=iterations))
        filtered, _ = V.denoise_variance(acc, cnt, mom, iterations, V.DEFAULTS, hits if guided else None, fmt_rgba8=True)
        targets.append((buf, present_ref.present_bytes(filtered, wt, ht, pitch, order, buf.nbytes, offset, FILL)))
    # tickets continue hrt_present's sequence
    assert tickets == [t0 + 1 + i for i in range(len(shots))]
    assert ctx.present(ACCUM, plain.ptr, plain.nbytes, w, h) == tickets[-1] + 1
    # work issued afterwards does not show in the targets
    ctx.trace(case.push(9))
    ctx.accumulate_history_moments(32)
    ctx.present_wait(ctx.present(TRACE, plain.ptr, plain.nbytes, w, h))
    for t in tickets:
        assert ctx.present_done(t)
    for k, (buf, want) in enumerate(targets):
        assert buf.read().tobytes() == want.tobytes(), shots[k]
    ctx.synchronize()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    for buf, _ in targets:
        buf.free()
    d_guide.free()
    plain.free()


# ---- 5. nothing else moves ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_the_old_entry_points_give_the_same_bytes_before_and_after(mode):
    """hrt_accumulate, hrt_compute_n, hrt_denoise, hrt_reproject and hrt_accumulate_history on a context that used the
    new calls (whose reprojection swapped the buffers of A, N and M) against a twin that never did; and the plain
    history calls leave the moments image alone."""
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, debug=True), case.context(mode=mode)
    hits = synthetic_guide(w, h)
    d_hits = DevBuf(w * h * 32).write(hits)
    views = view_pairs(size)[1]

    def old_calls(c, base):
        out = []
        for frame in range(2):
            c.trace(case.push(base + frame))
            c.accumulate(frame)
        c.compute_n(case.push(base + 5), 3)
        out.append(c.read(ACCUM, native(mode)))
        out.append(c.denoise(RGBA32F, d_hits.ptr))
        c.fill_history(3)
        c.reproject(views[1], d_hits.ptr, views[2], d_hits.ptr)
        c.trace(case.push(base + 9))
        c.accumulate_history(8)
        out.append(c.read(ACCUM, native(mode)))
        out.append(c.read_history())
        return out

    before = old_calls(ctx, 1)
    for a, b in zip(before, old_calls(twin, 1)):
        assert a.tobytes() == b.tobytes()
    # the new calls, with a reprojection in either direction and the filter
    ctx.fill_moments(0.5, 0.75)
    ctx.reproject_moments(views[1], d_hits.ptr, views[2], d_hits.ptr)
    ctx.trace(case.push(30))
    ctx.accumulate_history_moments(8)
    ctx.reproject_moments(views[2], d_hits.ptr, views[1], d_hits.ptr, filter=_lib.REPROJECT_NEAREST)
    ctx.denoise_variance(RGBA8, d_hits.ptr)
    moments = ctx.read_moments()
    after = old_calls(ctx, 40)
    for a, b in zip(after, old_calls(twin, 40)):
        assert a.tobytes() == b.tobytes()
    assert ctx.read_moments().tobytes() == moments.tobytes()  # none of the old calls touched the moments image
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    d_hits.free()


def test_fill_and_read_moments_round_trip_host_and_device():
    size = w, h = (37, 23)
    ctx = E.HrtContext(size, device=0, debug=True)
    dev = DevBuf(w * h * 8 + 64)
    for m1, m2 in ((0.0, 0.0), (1.5, -2.25), (float("inf"), 1e-30)):
        ctx.fill_moments(m1, m2)
        want = np.empty((h, w, 2), F32)
        want[..., 0], want[..., 1] = m1, m2
        assert equal(ctx.read_moments(), want)
        ctx.read_moments_into(dev.ptr, w * h * 8)
        raw = dev.read()
        assert raw[:w * h * 8].tobytes() == want.tobytes() and (raw[w * h * 8:] == FILL).all()
    assert (ctx.read_history() == 0).all()  # hrt_fill_moments leaves the counts alone
    assert ctx.check_guards()[1] == 0
    ctx.close()
    dev.free()


# ---- 6. the rejections ------------------------------------------------------------------------------------------------------

def test_rejections_enqueue_nothing_and_leave_the_context_usable():
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context()
    ctx.trace(case.push(1))
    ctx.accumulate_history_moments(4)
    lib, handle = ctx.lib, ctx.handle
    d_hits = DevBuf(w * h * 32 + 16)
    ctx.intersect_primary_into(case.push(), d_hits.ptr)
    view = E.View(case.camera, size, case.settings).record
    host = np.full(w * h * 16, FILL, np.uint8)
    host_v = np.full(w * h, 7.0, F32)
    target = DevBuf(w * h * 4)
    good, good_r = ctx.variance_info(), ctx.reproject_info()
    before = ctx.denoise_variance(RGBA32F, d_hits.ptr)
    t0 = ctx.present(ACCUM, target.ptr, target.nbytes, w, h)
    ctx.present_wait(t0)
    shown = target.read()
    state = (ctx.read(ACCUM), ctx.read_history(), ctx.read_moments(), ctx.stats().accumulates)
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731

    def raw(info=good, guide=d_hits.ptr, fmt=RGBA32F, dst=host.ctypes.data, nbytes=host.nbytes, vdst=host_v.ctypes.data,
            vbytes=host_v.nbytes):
        return lib.hrt_denoise_variance(handle, ref(info), ctypes.c_void_p(guide or 0), fmt, ctypes.c_void_p(dst or 0), nbytes,
                                        ctypes.c_void_p(vdst or 0), vbytes)

    def raw_present(info=good, guide=d_hits.ptr, image=ACCUM, dst=target.ptr, nbytes=target.nbytes, flags=0):
        pi, t = _lib.PresentInfo(image, _lib.PRESENT_B8G8R8A8, w, h, w * 4, flags), ctypes.c_uint64(99)
        st = lib.hrt_denoise_variance_present(handle, ref(info), ctypes.c_void_p(guide or 0), ctypes.byref(pi),
                                              ctypes.c_void_p(dst or 0), nbytes, ctypes.byref(t))
        assert t.value == 99
        return st

    def altered(**kw):
        info = ctx.variance_info()
        for k, v in kw.items():
            setattr(info, k, v)
        return info

    bad_infos = [("iterations", 6, b"iterations"), ("flags", 1, b"flags"), ("method", 3, b"method"),
                 ("method", 99, b"method"), ("min_history", 0, b"min_history")]
    bad_infos += [(s, v, b"finite") for s in ("sigma_variance", "variance_floor", "sigma_normal", "sigma_depth")
                  for v in (0.0, -1.0, float("nan"), float("inf"))]
    for call in (raw, raw_present):
        assert call(info=None) == 1 and b"null info" in lib.hrt_last_error(handle)
        for field, value, word in bad_infos:
            assert call(info=altered(**{field: value})) == 1, (field, value)
            err = lib.hrt_last_error(handle)
            assert b"hrt_denoise_variance" in err and word in err, (field, value, err)
        hits_host = np.zeros(w * h, dtype=_lib.HIT_DTYPE)
        assert call(guide=hits_host.ctypes.data) == 1 and b"guide" in lib.hrt_last_error(handle)   # host memory
        assert call(guide=d_hits.ptr + 8) == 1 and b"aligned" in lib.hrt_last_error(handle)         # misaligned
        assert call(dst=None) == 1
    assert raw(fmt=7) == 1 and b"format" in lib.hrt_last_error(handle)
    assert raw(nbytes=w * h * 16 - 1) == 1 and b"too small" in lib.hrt_last_error(handle)
    assert raw(vbytes=w * h * 4 - 1) == 1 and b"variance destination too small" in lib.hrt_last_error(handle)
    assert raw_present(nbytes=target.nbytes - 1) == 1
    assert raw_present(image=TRACE) == 1 and b"HRT_IMG_ACCUM" in lib.hrt_last_error(handle)
    assert raw_present(flags=1) == 1 and b"flags" in lib.hrt_last_error(handle)
    assert raw_present(dst=host.ctypes.data, nbytes=w * h * 4) == 1  # pageable host target
    assert (host == FILL).all() and (host_v == 7.0).all() and target.read().tobytes() == shown.tobytes()

    # what the shadowed history calls reject
    def raw_reproject(info=good_r, prev=view, prev_hits=d_hits.ptr, cur=view, cur_hits=d_hits.ptr):
        return lib.hrt_reproject_moments(handle, ref(info), ref(prev), ctypes.c_void_p(prev_hits or 0), ref(cur),
                                         ctypes.c_void_p(cur_hits or 0))

    def altered_r(**kw):
        info = ctx.reproject_info()
        for k, v in kw.items():
            setattr(info, k, v)
        return info

    for kw in (dict(info=None), dict(prev=None), dict(cur=None), dict(prev_hits=None), dict(cur_hits=None)):
        assert raw_reproject(**kw) == 1 and b"hrt_reproject_moments: null" in lib.hrt_last_error(handle), kw
    for field, value, word in (("filter", 2, b"filter"), ("flags", 1, b"flags"), ("depth_tolerance", -0.01, b"tolerance"),
                               ("depth_tolerance", float("nan"), b"tolerance"),
                               ("min_normal_dot", float("nan"), b"min_normal_dot")):
        assert raw_reproject(info=altered_r(**{field: value})) == 1 and word in lib.hrt_last_error(handle), (field, value)
    host_raw = np.zeros(w * h * 32 + 16, np.uint8)
    host_hits = host_raw.ctypes.data + (-host_raw.ctypes.data) % 16
    for which in ("prev_hits", "cur_hits"):
        assert raw_reproject(**{which: host_hits}) == 1 and b"device" in lib.hrt_last_error(handle)
        assert raw_reproject(**{which: d_hits.ptr + 8}) == 1 and b"aligned" in lib.hrt_last_error(handle)
    for bad in (0, CAP + 1, 2**32 - 1):
        assert lib.hrt_accumulate_history_moments(handle, bad) == 1
        assert b"hrt_accumulate_history_moments: max_history" in lib.hrt_last_error(handle)
    small = np.full(w * h * 2, 7.0, F32)
    assert lib.hrt_read_moments(handle, _lib.ptr(small), small.nbytes - 1) == 1 and b"too small" in lib.hrt_last_error(handle)
    assert lib.hrt_read_moments(handle, None, small.nbytes) == 1 and b"null" in lib.hrt_last_error(handle)
    assert (small == 7.0).all()
    # nothing was enqueued or issued: the state and the next ticket are as they were, and the calls still work
    assert ctx.read(ACCUM).tobytes() == state[0].tobytes() and ctx.read_history().tobytes() == state[1].tobytes()
    assert ctx.read_moments().tobytes() == state[2].tobytes() and ctx.stats().accumulates == state[3]
    assert ctx.present(ACCUM, target.ptr, target.nbytes, w, h) == t0 + 1
    assert ctx.denoise_variance(RGBA32F, d_hits.ptr).tobytes() == before.tobytes()
    assert raw(info=altered(iterations=0, min_history=2**32 - 1), vdst=None, vbytes=0) == 0  # the edges of the ranges
    ctx.close()
    # a row-tile partition, with and without a communicator, and an unpartitioned context joined to one
    parts = [case.context(partition=(8, p, 2)) for p in range(2)]
    view_py = E.View(case.camera, size, case.settings)
    for joined in (False, True):
        if joined:
            E.HrtContext.comm_init_all(parts)
        for c in parts:
            for call in (lambda: c.reproject_moments(view_py, d_hits.ptr, view_py, d_hits.ptr),
                         lambda: c.accumulate_history_moments(4), lambda: c.fill_moments(0.0, 0.0), c.read_moments,
                         lambda: c.denoise_variance(RGBA8), lambda: c.denoise_variance_present(target.ptr, target.nbytes, w, h)):
                with pytest.raises(_lib.HrtError, match="partition"):
                    call()
    for c in parts:
        c.close()
    single = case.context()
    E.HrtContext.comm_init_all([single])
    for call in (lambda: single.accumulate_history_moments(4), lambda: single.denoise_variance(RGBA8),
                 lambda: single.reproject_moments(view_py, d_hits.ptr, view_py, d_hits.ptr)):
        with pytest.raises(_lib.HrtError, match="communicator"):
            call()
    single.close()
    d_hits.free()
    target.free()


# ---- 7. the mirrors --------------------------------------------------------------------------------------------------------

def _demo_sequence(settings, size):
    """What tests/cpp/variance_demo.cpp does, through the Python mirror: (moments after the last fold, the filtered
    image, the filtered variance, the target's bytes), each checked against the numpy chain."""
    w, h = size
    ctx = E.HrtContext(size, device=0, mode=_lib.MODE_RGBA32F)
    pipe, diffuse = E.RayTracePipeline(ctx, size, settings), E.DiffusePipeline(ctx, size)
    before, after = E.Camera(), E.Camera([0.05, 0.02, -0.03], [1.0, 0.03, 0.08])
    acc, cnt, mom = np.zeros((h, w, 4), F32), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    for frame in range(3):
        pipe.compute(before, frame)
        diffuse.next_frame_history(pipe.image(), moments=True)
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, ctx.read(TRACE, RGBA32F), 32)
    d_hits = [DevBuf(w * h * 32), DevBuf(w * h * 32)]
    pipe.first_hits_into(before, d_hits[0].ptr)
    pipe.first_hits_into(after, d_hits[1].ptr)
    hp, hc = (d.read().view(_lib.HIT_DTYPE).reshape(h, w) for d in d_hits)
    vp, vc = E.View(before, size, settings), E.View(after, size, settings)
    ctx.reproject_moments(vp, d_hits[0].ptr, vc, d_hits[1].ptr)
    acc, cnt, mom = V.reproject_moments(acc, cnt, mom, vp.record, hp, vc.record, hc, H.BILINEAR, *H.DEFAULTS)
    assert 0 < (cnt == 0).sum() < cnt.size
    for frame in range(3, 5):
        pipe.compute(after, frame)
        diffuse.next_frame_history(pipe.image(), moments=True)
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, ctx.read(TRACE, RGBA32F), 32)
    moments = ctx.read_moments()
    assert equal(moments, mom) and equal(ctx.read(ACCUM, RGBA32F), acc) and equal(ctx.read_history(), cnt)
    filtered, variance = ctx.denoise_variance(RGBA32F, d_hits[1].ptr, with_variance=True)
    want, wantv = V.denoise_variance(acc, cnt, mom, 5, V.DEFAULTS, hc)
    assert equal(filtered, want) and equal(variance, wantv), report(filtered, want)
    assert equal(diffuse.variance_denoised(d_hits[1].ptr, RGBA32F), want)
    target = DevBuf(w * h * 4)
    rp = E.RenderPassOverFrame(ctx)
    pt = E.PresentTarget(target.ptr, target.nbytes, w, h)
    ctx.present_wait(rp.render_variance_denoised(diffuse.image(), pt, d_hits[1].ptr))
    shown = target.read()
    want8, _ = V.denoise_variance(acc, cnt, mom, 5, V.DEFAULTS, hc, fmt_rgba8=True)
    assert shown.tobytes() == present_ref.present_pixels(want8, w, h, present_ref.B8G8R8A8).tobytes()
    with pytest.raises(ValueError):
        rp.render_variance_denoised(pipe.image(), pt)  # the trace image has no moments
    ctx.close()
    for d in d_hits + [target]:
        d.free()
    return moments, filtered, variance, shown


def test_python_and_cpp_mirrors(tmp_path):
    """HrtContext.reproject_moments / denoise_variance, DiffusePipeline.next_frame_history(moments=True) /
    variance_denoised and RenderPassOverFrame.render_variance_denoised against the numpy chain, and include/hrt_app.hpp's
    counterparts (tests/cpp/variance_demo) against the Python mirror's bytes on the box scene's geometry."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "variance_demo.mk"], check=True)  # (up to date after build())
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
    r = subprocess.run([os.path.join(cpp, "variance_demo"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    w, h = 48, 32
    n = w * h
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [w, h] and len(raw) == 8 + n * (8 + 16 + 4 + 4)
    moments = np.frombuffer(raw[8:8 + n * 8], F32).reshape(h, w, 2)
    filtered = np.frombuffer(raw[8 + n * 8:8 + n * 24], F32).reshape(h, w, 4)
    variance = np.frombuffer(raw[8 + n * 24:8 + n * 28], F32).reshape(h, w)
    shown = np.frombuffer(raw[8 + n * 28:], np.uint8)
    # the demo's scene through the Python mirror: the same geometry, Lambertian grey, 1 sample, 4 bounces, light on
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    st = E.RayTracerSettings(num_samples=1, max_bounces=4, use_environment_lighting=True,
                             sphere_data=[E.Sphere(s.centre, s.radius, grey) for s in settings.sphere_data],
                             mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in settings.mesh_data])
    want = _demo_sequence(st, (w, h))
    assert equal(moments, want[0]) and equal(filtered, want[1]) and equal(variance, want[2])
    assert shown.tobytes() == want[3].tobytes()
