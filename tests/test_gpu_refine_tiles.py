"""Tile-masked refinement on the device (hrt_refine_tiles, hrt_refine_tiles_until): every byte of
the accumulator, the count image and the moments image against a twin context that ran hrt_refine(FRAME) frame by frame;
that the launches really skip the unselected tiles (the segment and triangle-test counts are the CPU oracle's sums over
the selected tiles' pixels); what the pass leaves in the trace image; that lane 0's plan is read and never written; that
the bytes do not depend on the plan; the until loop; the rejections; and the Python and C++ mirrors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pyoracle
import refine_ref as R
import refine_tiles_ref as T
from helpers import E, SceneCase, _lib
from test_gpu_history import CAP, DevBuf, synthetic_source
from test_gpu_refine import FILL, FRAME, MODES, check_state, equal, mixed_history, native, read_state, report

pytestmark = pytest.mark.gpu

F32 = np.float32
TRACE, ACCUM = _lib.IMG_TRACE, _lib.IMG_ACCUM
# 1x1; 7x5: one partial tile; 37x23: 5x3 tiles, partial right and bottom, a partial last mask word; 130x70: rows that
# straddle words, 153 tiles
SIZES = [(1, 1), (7, 5), (37, 23), (130, 70)]
SCENES = {(1, 1): "box", (7, 5): "spheres", (37, 23): "box", (130, 70): "box"}
VARIANTS = [_lib.KERNEL_BUNDLE_CULL_LDS, _lib.KERNEL_BUNDLE_BVH_LDS, _lib.KERNEL_BUNDLE_WQ, 10, _lib.KERNEL_AUTO]
PERSISTENT = {7, 8, 9, 10}  # hrt_launch_plan.h kKernelTraits


def masks_of(w, h, seed=9):
    """(name, selection): none, all, the first pixel, the last pixel, one whole tile, one pixel in each corner tile, one
    pixel per tile in alternate tiles, random 5 % and 50 %."""
    rng = np.random.default_rng([seed, w, h])
    y, x = np.mgrid[0:h, 0:w]
    tx, ty = x >> 3, y >> 3
    ntx, nty = (w + 7) // 8, (h + 7) // 8
    tile = (tx == min(1, ntx - 1)) & (ty == min(1, nty - 1))
    corners = ((x == 0) | (x == w - 1)) & ((y == 0) | (y == h - 1))
    # the pixel (3, 5) of the tile, or the tile's last real pixel where the edge cuts it short
    px, py = np.minimum(tx * 8 + 3, w - 1), np.minimum(ty * 8 + 5, h - 1)
    alternate = ((tx + ty) % 2 == 0) & (x == px) & (y == py)
    return [("none", x < 0), ("all", x >= 0), ("first", (x == 0) & (y == 0)), ("last", (x == w - 1) & (y == h - 1)),
            ("tile", tile), ("corners", corners), ("alternate tiles", alternate), ("5 %", rng.uniform(size=(h, w)) < 0.05),
            ("50 %", rng.uniform(size=(h, w)) < 0.5)]


def host_words(name, sel):
    words = R.pack_mask(sel)
    n = sel.size
    if name == "last" and n % 32:  # bits of the last word beyond the image are ignored
        words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    return words


def check_stats(st, sel, variant, frames, what):
    tiles, tsel, nsel, traced = T.counts(sel)
    assert st.reserved == 0 and st.selected == nsel, (what, st.selected, nsel)
    if nsel == 0:
        assert (st.kernel_ran, st.whole_frame, st.tiles, st.tiles_selected, st.items, st.pixels_traced) == (0,) * 6, what
        return
    assert st.whole_frame == (0 if st.kernel_ran in PERSISTENT else 1), (what, st.kernel_ran, st.whole_frame)
    assert (st.tiles, st.tiles_selected) == (tiles, tsel), (what, st.tiles, st.tiles_selected, tiles, tsel)
    if st.whole_frame:
        assert st.pixels_traced == sel.size and st.items == 0, what
    else:
        assert st.pixels_traced == traced and tsel <= st.items <= 64 * tsel, (what, st.pixels_traced, traced, st.items)
    if variant == _lib.KERNEL_AUTO:
        assert st.whole_frame == 1, (what, "AUTO resolves to a non-persistent kernel on these scenes", st.kernel_ran)


# ---- 1. state against a twin ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("size", SIZES)
def test_state_against_a_twin_that_refined_frame_by_frame(size, variant, mode):
    w, h = size
    case = SceneCase(SCENES[size], size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, variant=variant, debug=True), case.context(mode=mode, variant=variant)
    src = synthetic_source(w, h, mode)
    words = (w * h + 31) // 32
    dev = DevBuf(words * 4 + 64)
    everything = R.pack_mask(np.ones((h, w), bool))
    cap, first = 8, 11
    masks = masks_of(w, h)
    seen_masked = False
    for count, (m1, m2) in ((0, (9.0, 9.0)), (3, (0.4, 0.9)), (8, (2.5, 0.125))):  # none, below the cap, at the cap
        before = (src, np.full((h, w), count, np.uint32), np.empty((h, w, 2), F32))
        before[2][..., 0], before[2][..., 1] = m1, m2

        def restore(c):
            c.load_accumulator(src)
            c.fill_history(count)
            c.fill_moments(m1, m2)

        # the twin: hrt_refine(FRAME) frame by frame; a pixel's fold does not look at its neighbours (S17), so the
        # twin's pass over every pixel gives each mask's expected bytes -- and one mask is run on the twin as it is
        after = {}
        restore(twin)
        for f in range(3):
            twin.refine(case.push(first + f), everything, cap, FRAME)
            if f in (0, 2):
                after[f + 1] = read_state(twin, mode)
        for frames in (1, 3):
            literal = dict(masks)["50 %"]
            restore(twin)
            for f in range(frames):
                twin.refine(case.push(first + f), R.pack_mask(literal), cap, FRAME)
            want = tuple(np.where(literal.reshape(literal.shape + (1,) * (a.ndim - 2)), a, b) for a, b in zip(after[frames], before))
            check_state(twin, mode, want, (count, frames, "the twin's own masked passes"))
        for k, (name, sel) in enumerate(masks):
            host = host_words(name, sel)
            dev.write(host)
            for frames in (1, 3):
                want = tuple(np.where(sel.reshape(sel.shape + (1,) * (a.ndim - 2)), a, b) for a, b in zip(after[frames], before))
                for moments in (True, False):
                    what = (count, name, frames, moments)
                    restore(ctx)
                    st = ctx.refine_tiles(case.push(first), dev.ptr if (k + frames + moments) & 1 else host, cap, frames,
                                          moments=moments)
                    check_state(ctx, mode, (want[0], want[1], want[2] if moments else before[2]), what)
                    check_stats(st, sel, variant, frames, what)
                    seen_masked |= st.selected != 0 and st.whole_frame == 0
        assert (dev.read()[words * 4:] == FILL).all()
    if variant == _lib.KERNEL_BUNDLE_CULL_LDS and size == (37, 23):
        assert seen_masked, "variant 7 on box 37x23 runs the masked path"
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    dev.free()


# ---- 2. skipping is real --------------------------------------------------------------------------------------------

def stat_tuple(ctx):
    s = ctx.stats()
    return s.segments, s.tri_tests, s.traces, s.accumulates


@pytest.mark.parametrize("variant", [_lib.KERNEL_BUNDLE_CULL_LDS, _lib.KERNEL_BUNDLE_WQ])
def test_only_the_selected_tiles_are_traced(variant):
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context(variant=variant, debug=True, options={_lib.OPT_FOLD_RECORDS: 1})
    ctx.trace(case.push(1))
    ctx.accumulate(0)
    target = DevBuf(w * h * 4)
    t0 = ctx.present(ACCUM, target.ptr, target.nbytes, w, h)
    records = ctx.fold_records(with_total=True)
    frames, first = 3, 21
    whole = None
    for name in ("all", "alternate tiles", "corners", "tile"):
        sel = dict(masks_of(w, h))[name]
        ys, xs = np.nonzero(T.traced_pixels(sel))
        seg = tests = 0
        for f in range(frames):
            _, s, t = pyoracle.trace_pixels(case.push(first + f), case.rays, case.spheres, case.tris, case.meshes, xs, ys)
            seg, tests = seg + s, tests + t
        s0 = stat_tuple(ctx)
        st = ctx.refine_tiles(case.push(first), R.pack_mask(sel), CAP, frames)
        s1 = stat_tuple(ctx)
        assert st.whole_frame == 0 and st.kernel_ran == variant
        assert (st.tiles, st.tiles_selected, st.selected, st.pixels_traced) == T.counts(sel), name
        assert (s1[0] - s0[0], s1[1] - s0[1]) == (seg, tests), (name, s1[0] - s0[0], seg, s1[1] - s0[1], tests)
        assert s1[2] == s0[2] + frames and s1[3] == s0[3], name
        last = ctx.stats()
        assert (last.last_kernel, last.last_frames) == (variant, frames)
        if name == "all":
            whole = (seg, tests)
        else:
            assert seg < whole[0] and tests <= whole[1], (name, "a sparse mask costs less than the frame", seg, whole)
    after = ctx.fold_records(with_total=True)
    assert after[1] == records[1] and after[0].tobytes() == records[0].tobytes()
    assert ctx.present(ACCUM, target.ptr, target.nbytes, w, h) == t0 + 1  # no ticket was taken in between
    assert ctx.check_guards()[1] == 0
    ctx.close()
    target.free()


# ---- 3. the trace image ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", [_lib.KERNEL_BUNDLE_CULL_LDS, _lib.KERNEL_BUNDLE_WQ])
def test_the_trace_image_holds_the_last_frame_in_the_selected_tiles_only(variant, mode):
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context(mode=mode, variant=variant, debug=True, options={_lib.OPT_OVERLAP: 1})
    twin = case.context(mode=mode, variant=variant)
    a, b = 5, 30
    for frames in (3, 1):
        twin.trace(case.push(b + frames - 1))
        new = twin.read(TRACE, native(mode))
        for name in ("alternate tiles", "corners", "5 %"):
            sel = dict(masks_of(w, h))[name]
            ctx.trace(case.push(a))
            old = ctx.read(TRACE, native(mode))
            st = ctx.refine_tiles(case.push(b), R.pack_mask(sel), CAP, frames)
            assert st.whole_frame == 0
            traced = T.traced_pixels(sel)
            assert not traced.all() or name == "5 %"
            want = np.where(traced[..., None], new, old)
            got = ctx.read(TRACE, native(mode))
            assert equal(got, want), (name, frames, report(got, want))
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()


# ---- 4. lane 0's plan -----------------------------------------------------------------------------------------------

def tile_costs(ctx, tiles):
    out = np.zeros(tiles + 16, np.uint32)
    _lib.check(ctx.lib.hrt_debug_tile_costs(ctx.handle, ctypes.c_void_p(out.ctypes.data), out.size), "tile costs", ctx.handle,
               ctx.lib)
    return out


@pytest.mark.parametrize("variant", [_lib.KERNEL_BUNDLE_CULL_LDS, _lib.KERNEL_BUNDLE_WQ])
def test_lane_0s_costs_and_plan_are_left_alone(variant):
    size = w, h = (130, 70)
    mode = _lib.MODE_RGBA8
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(variant=variant, debug=True), case.context(variant=variant)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    sel = dict(masks_of(w, h))["alternate tiles"]
    for c in (ctx, twin):
        c.compute_n(case.push(1), 4)
    before = tile_costs(ctx, tiles)
    assert (before[:tiles] > 0).all()
    st = ctx.refine_tiles(case.push(40), R.pack_mask(sel), CAP, 3)
    assert st.whole_frame == 0
    assert tile_costs(ctx, tiles).tobytes() == before.tobytes()
    # the twin refines frame by frame (its traces rewrite its costs: the plans differ, the bytes do not)
    for f in range(3):
        twin.refine(case.push(40 + f), R.pack_mask(sel), CAP, FRAME)
    for c in (ctx, twin):
        c.compute_n(case.push(60), 3)
    check_state(ctx, mode, read_state(twin, mode), "after the pass and a later hrt_compute_n")
    assert ctx.read(TRACE, native(mode)).tobytes() == twin.read(TRACE, native(mode)).tobytes()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()


# ---- 5. the bytes do not depend on the plan -----------------------------------------------------------------------------

def sky_units(ctx):
    v = ctypes.c_uint64()
    ctx._check(ctx.lib.hrt_debug_sky_units(ctx.handle, ctypes.byref(v)), "hrt_debug_sky_units")
    return v.value


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant,options", [
    (_lib.KERNEL_BUNDLE_CULL_LDS, {}),
    (_lib.KERNEL_BUNDLE_WQ, {}),
    (_lib.KERNEL_BUNDLE_WQ, {_lib.OPT_SPLIT: 8, _lib.OPT_SPLIT_FACTOR: 0}),
    (_lib.KERNEL_BUNDLE_CULL_LDS, {_lib.OPT_COOP: 1}),
    (_lib.KERNEL_BUNDLE_WQ, {_lib.OPT_SKY_LANE: 1}),
])
def test_the_bytes_do_not_depend_on_the_plan(variant, options, mode):
    size = w, h = (130, 70)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, variant=variant, options=options, debug=True), case.context(mode=mode)
    frames = 3
    for name in ("alternate tiles", "50 %"):
        sel = dict(masks_of(w, h))[name]
        mask = R.pack_mask(sel)
        tsel = T.counts(sel)[1]
        for c in (ctx, twin):
            c.fill_history(0)
        # a pass before any trace of this context plans from a cost of 1 per tile; after hrt_compute_n from lane 0's
        for step, first in enumerate((10, 20)):
            u0 = sky_units(ctx)
            st = ctx.refine_tiles(case.push(first), mask, CAP, frames)
            assert st.whole_frame == 0 and st.tiles_selected == tsel
            grown = sky_units(ctx) - u0
            assert grown <= tsel * frames, (grown, tsel, frames)  # trace_sky takes sky items of the masked plan at most
            if not options.get(_lib.OPT_SKY_LANE):
                assert grown == 0
            for f in range(frames):
                twin.refine(case.push(first + f), mask, CAP, FRAME)
            check_state(ctx, mode, read_state(twin, mode), (name, options, "costs valid" if step else "uniform costs"))
            if step == 0:
                saved = read_state(ctx, mode)
                ctx.compute_n(case.push(90), 2)  # lane 0 records its costs
                ctx.load_accumulator(saved[0])
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()


def test_diagnostics_fall_back_to_whole_frames():
    """HRT_OPT_COUNTERS = 2 on a persistent kernel: whole_frame = 1, the same state, the last frame whole in the trace
    image."""
    size = w, h = (37, 23)
    mode = _lib.MODE_RGBA8
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context(variant=_lib.KERNEL_BUNDLE_WQ, options={_lib.OPT_COUNTERS: 2}, debug=True)
    twin = case.context(variant=_lib.KERNEL_BUNDLE_WQ)
    sel = dict(masks_of(w, h))["alternate tiles"]
    for frames, first in ((3, 10), (1, 20)):
        st = ctx.refine_tiles(case.push(first), R.pack_mask(sel), CAP, frames)
        assert (st.whole_frame, st.kernel_ran, st.items, st.pixels_traced) == (1, _lib.KERNEL_BUNDLE_WQ, 0, w * h)
        assert (st.tiles, st.tiles_selected, st.selected) == T.counts(sel)[:3]
        for f in range(frames):
            twin.refine(case.push(first + f), R.pack_mask(sel), CAP, FRAME)
        check_state(ctx, mode, read_state(twin, mode), ("diagnostics", frames))
        assert ctx.read(TRACE, native(mode)).tobytes() == twin.read(TRACE, native(mode)).tobytes()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()


# ---- 6. the until loop ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,size,variant", [("box", (37, 23), _lib.KERNEL_BUNDLE_CULL_LDS),
                                               ("box", (130, 70), _lib.KERNEL_BUNDLE_WQ),
                                               ("spheres", (64, 64), _lib.KERNEL_AUTO)])
def test_refine_tiles_until(name, size, variant, mode):
    w, h = size
    case = SceneCase(name, size, num_samples=1, max_bounces=2)
    ctx, twin = case.context(mode=mode, variant=variant, debug=True), case.context(mode=mode, variant=variant)
    d_hits = DevBuf(w * h * 32)
    ctx.intersect_primary_into(case.push(), d_hits.ptr)
    key = R.keys_of(d_hits.read().view(_lib.HIT_DTYPE), (h, w))
    acc, cnt, mom = mixed_history(ctx, case, mode)
    mixed_history(twin, case, mode)
    rule = dict(min_history=5, max_count=9, radius=1, tolerance=0.05, luminance_floor=0.01)
    # frames_per_pass = 1: hrt_refine_until(FRAME) on the twin, output for output and byte for byte
    got = ctx.refine_tiles_until(case.push(40), CAP, 4, 1, d_hits.ptr, **rule)
    assert got == twin.refine_until(case.push(40), CAP, 4, d_hits.ptr, FRAME, **rule) and got[0] == 4
    check_state(ctx, mode, read_state(twin, mode), "frames_per_pass 1")
    # frames_per_pass = 3 against the numpy chain, from the same start
    acc, cnt, mom = read_state(ctx, mode)
    cache = {}

    def frames(j):
        if j not in cache:
            twin.trace(case.push(60 + j))
            cache[j] = twin.read(TRACE, native(mode))
        return cache[j]

    loose = (2, 11, 1, 1e-6, 0.01)  # everything under the budget is selected: the passes run into max_count
    want = T.refine_tiles_until(acc, cnt, mom, frames, CAP, 3, 3, None, loose)
    got = ctx.refine_tiles_until(case.push(60), CAP, 3, 3, None, min_history=2, max_count=11, tolerance=1e-6)
    assert got == (want[3], want[4], want[5]) and want[3] >= 2 and want[4] == 3 * sum(want[6])
    check_state(ctx, mode, want[:3], "frames_per_pass 3")
    assert int(want[1].max()) > 11  # a pixel passes max_count by up to frames_per_pass - 1
    assert ctx.refine_tiles_until(case.push(90), CAP, 4, 2, d_hits.ptr, min_history=1, max_count=1) == (0, 0, True)
    assert ctx.refine_tiles_until(case.push(90), CAP, 0, 2) == (0, 0, False)
    check_state(ctx, mode, want[:3], "settled")
    assert ctx.check_guards()[1] == 0
    ctx.close()
    twin.close()
    d_hits.free()


# ---- 7. the rejections ------------------------------------------------------------------------------------------------

def test_rejections_enqueue_nothing_and_leave_the_context_usable():
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context(variant=_lib.KERNEL_BUNDLE_CULL_LDS, debug=True)
    ctx.trace(case.push(1))
    ctx.accumulate_history_moments(4)
    lib, handle = ctx.lib, ctx.handle
    words = (w * h + 31) // 32
    d_hits, d_mask = DevBuf(w * h * 32 + 16), DevBuf(words * 4 + 16)
    ctx.intersect_primary_into(case.push(), d_hits.ptr)
    state, st0 = read_state(ctx, ctx.mode), ctx.stats()
    mask = np.full(words, 0xFFFFFFFF, np.uint32)
    stats = _lib.RefineTilesStats()
    passes, frames, settled = ctypes.c_uint32(5), ctypes.c_uint64(5), ctypes.c_uint32(5)
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    err = lambda: lib.hrt_last_error(handle)  # noqa: E731

    def tiles(pc=case.push(5), m=mask.ctypes.data, max_history=8, n=2, flags=1):
        return lib.hrt_refine_tiles(handle, ref(pc), ctypes.c_void_p(m or 0), max_history, n, flags, ctypes.byref(stats))

    def until(pc=case.push(5), rule=ctx.refine_rule(), guide=d_hits.ptr, max_history=8, n=2, flags=0, out=passes, out2=frames):
        return lib.hrt_refine_tiles_until(handle, ref(pc), ref(rule), ctypes.c_void_p(guide or 0), max_history, 4, n, flags,
                                          ref(out), ref(out2), ctypes.byref(settled))

    assert tiles(pc=None) == 1 and b"null" in err()
    assert tiles(m=None) == 1 and b"null" in err()
    assert until(pc=None) == 1 and b"null" in err()
    assert until(rule=None) == 1 and b"null" in err()
    assert until(out=None) == 1 and b"null" in err()
    assert until(out2=None) == 1 and b"null" in err()
    for bad in (0, _lib.REFINE_TILES_MAX_FRAMES + 1, 2**32 - 1):
        assert tiles(n=bad) == 1 and b"frames" in err()
        assert until(n=bad) == 1 and b"frames" in err()
    assert tiles(flags=2) == 1 and b"flag" in err()
    assert until(flags=2) == 1 and b"flag" in err()
    assert tiles(m=d_mask.ptr + 2) == 1 and b"aligned" in err()
    assert until(guide=d_hits.ptr + 8) == 1 and b"aligned" in err()
    for bad in (0, CAP + 1, 2**32 - 1):
        assert tiles(max_history=bad) == 1 and b"max_history" in err()
        assert until(max_history=bad) == 1 and b"max_history" in err()
    for change, word in ((dict(init=1), b"init"), (dict(width=w + 1), b"width"), (dict(height=h - 1), b"width"),
                         (dict(num_spheres=99), b"exceed"), (dict(num_meshes=99), b"exceed")):
        pc = case.push(5)
        for k, v in change.items():
            setattr(pc, k, v)
        assert tiles(pc=pc) == 1 and word in err(), change
        assert until(pc=pc) == 1 and word in err(), change
    rule = ctx.refine_rule()
    rule.radius = 4
    assert until(rule=rule) == 1 and b"radius" in err()
    # hrt_refine's method argument did not grow a value
    assert lib.hrt_refine(handle, ref(case.push(5)), ctypes.c_void_p(mask.ctypes.data), 8, 3, 0, 1, None) == 1
    assert b"unknown method" in err()
    # nothing was enqueued or written
    assert all(a.tobytes() == b.tobytes() for a, b in zip(read_state(ctx, ctx.mode), state))
    st1 = ctx.stats()
    assert (st1.traces, st1.accumulates, st1.segments) == (st0.traces, st0.accumulates, st0.segments)
    assert (passes.value, frames.value, settled.value) == (5, 5, 5) and (d_mask.read() == FILL).all()
    # the edges of the accepted ranges, and the calls still work; NULL stats are accepted
    assert tiles(max_history=CAP, n=1) == 0 and stats.selected == w * h and stats.whole_frame == 0
    assert lib.hrt_refine_tiles(handle, ref(case.push(9)), ctypes.c_void_p(mask.ctypes.data), 8, 2, 0, None) == 0
    assert until() == 0
    assert ctx.check_guards()[1] == 0
    ctx.close()
    bare = E.HrtContext(size, device=0)
    with pytest.raises(_lib.HrtError, match="HRT_ERR_NO_SCENE"):
        bare.refine_tiles(case.push(5), mask, 8)
    with pytest.raises(_lib.HrtError, match="HRT_ERR_NO_SCENE"):
        bare.refine_tiles_until(case.push(5), 8, 2)
    bare.close()
    # a row-tile partition, and an unpartitioned context joined to a communicator
    parts = [case.context(partition=(8, p, 2)) for p in range(2)]
    for c in parts:
        for call in (lambda: c.refine_tiles(case.push(5), mask, 8), lambda: c.refine_tiles_until(case.push(5), 8, 2)):
            with pytest.raises(_lib.HrtError, match="partition"):
                call()
        c.close()
    single = case.context()
    E.HrtContext.comm_init_all([single])
    for call in (lambda: single.refine_tiles(case.push(5), mask, 8), lambda: single.refine_tiles_until(case.push(5), 8, 2)):
        with pytest.raises(_lib.HrtError, match="communicator"):
            call()
    single.close()
    d_hits.free()
    d_mask.free()


# ---- 8. the mirrors ---------------------------------------------------------------------------------------------------

def test_python_and_cpp_mirrors(tmp_path):
    """tests/cpp/refine_tiles_demo (include/hrt_app.hpp's Context::refine_tiles / refine_tiles_until) against the Python
    mirror's bytes for the same short sequence on the box scene's geometry, and the Python mirror against the numpy
    chain."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "refine_tiles_demo.mk"], check=True)  # (up to date after build())
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
    r = subprocess.run([os.path.join(cpp, "refine_tiles_demo"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    w, h = 48, 32
    head = np.frombuffer(raw[:64], np.uint64)
    assert head[:2].tolist() == [w, h] and len(raw) == 64 + w * h * (4 + 16)
    counts = np.frombuffer(raw[64:64 + w * h * 4], np.uint32).reshape(h, w)
    acc = np.frombuffer(raw[64 + w * h * 4:], F32).reshape(h, w, 4)
    # the demo's sequence through the Python mirror: Lambertian grey, 1 sample, 4 bounces, light on, variant 9
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    st = E.RayTracerSettings(num_samples=1, max_bounces=4, use_environment_lighting=True,
                             sphere_data=[E.Sphere(s.centre, s.radius, grey) for s in settings.sphere_data],
                             mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in settings.mesh_data])
    size = (w, h)
    ctx, twin = (E.HrtContext(size, device=0, mode=_lib.MODE_RGBA32F) for _ in range(2))
    for c in (ctx, twin):
        c.set_option(_lib.OPT_KERNEL_VARIANT, _lib.KERNEL_BUNDLE_WQ)
    pipe, diffuse, tpipe = E.RayTracePipeline(ctx, size, st), E.DiffusePipeline(ctx, size), E.RayTracePipeline(twin, size, st)
    cam = E.Camera([3.0, 1.5, 2.0], [-0.8, -0.3, -0.6])
    a, c, m = np.zeros((h, w, 4), F32), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    # a mask of the left half's pixels, two frames; then the until loop, two frames per pass, two passes
    sel = np.zeros((h, w), bool)
    sel[:, :w // 2] = True
    tiles = ctx.refine_tiles(pipe.push_constants(cam, 0, False), R.pack_mask(sel), 1 << 24, 2)

    def frames(j):
        tpipe.compute(cam, j)
        return twin.read(TRACE, _lib.FMT_RGBA32F)

    a, c, m = T.refine_tiles(a, c, m, [frames(0), frames(1)], sel, 1 << 24)
    want = T.refine_tiles_until(a, c, m, lambda j: frames(2 + j), 1 << 24, 2, 2)
    got = diffuse.refine_tiles_until(pipe, cam, 2, 2, 2)
    assert got == (want[3], want[4], want[5]) and got[0] == 2
    state = ctx.read(ACCUM, _lib.FMT_RGBA32F), ctx.read_history()
    assert equal(state[1], want[1]) and equal(state[0], want[0]), report(state[0], want[0])
    assert head[2:8].tolist() == [tiles.tiles, tiles.tiles_selected, tiles.selected, tiles.pixels_traced, got[0], got[1]]
    assert tiles.whole_frame == 0 and (tiles.tiles, tiles.tiles_selected) == T.counts(sel)[:2]
    assert equal(counts, state[1]) and equal(acc, state[0]), report(acc, state[0])
    ctx.close()
    twin.close()
