"""Fold records (HRT_OPT_FOLD_RECORDS, hrt_get_fold_records) and hrt_compute_until on the device.

Every expected record comes from numpy (tests/fold_ref.py) on read-backs of an INDEPENDENT context driven
by the existing hrt_trace / hrt_accumulate / hrt_read_image path with the option off -- the displayed image
(hrt_read_image(HRT_FMT_RGBA8)) before and after each fold, over the real rows -- or from the CPU oracle
alone; never from the code under test.  References are computed once per case and shared."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import epq_raytracer_amd as E
import fold_ref
from epq_raytracer_amd import _lib
from epq_raytracer_amd.pipeline import HrtContext
from helpers import SceneCase
from test_gpu_present import BGRA, Target

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = fold_ref.ANY
RGBA8, RGBA32F = _lib.MODE_RGBA8, _lib.MODE_RGBA32F


def native(mode):
    return _lib.FMT_RGBA8 if mode == RGBA8 else _lib.FMT_RGBA32F


def rec_tuples(recs):
    """(frame, changed_pixels, abs_delta_sum, max_delta) per record of HrtContext.fold_records()."""
    assert not recs["reserved"].any()
    return [(int(r["frame"]), int(r["changed_pixels"]), int(r["abs_delta_sum"]), int(r["max_delta"])) for r in recs]


def seeded(size, partition):
    """Cases whose accumulator starts from random texels: the strips and the single pixel, which see little
    of the box (300x1 renders black), so that every fold changes bytes -- and the partition, so that its
    padding rows change under a fold too and a kernel that counted them would report more."""
    return size[0] * size[1] < 500 or partition is not None


def seed_accumulator(ctx, size, mode):
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    shape = (ctx.local_rows, ctx.width, 4)
    if mode == RGBA8:
        ctx.load_accumulator(rng.integers(0, 256, shape, dtype=np.uint8))
    else:
        ctx.load_accumulator(rng.uniform(-0.1, 1.1, shape).astype(np.float32))


def state(ctx, mode):
    """(accumulator, trace image, counters): the images' real rows in the context's own format.  (The padding
    rows of a row-tile part are never shown, and a multi-frame launch leaves them unspecified.)"""
    st = ctx.stats()
    real = ctx.global_rows() < ctx.height
    return (ctx.read(_lib.IMG_ACCUM, native(mode))[real].view(np.uint8),
            ctx.read(_lib.IMG_TRACE, native(mode))[real].view(np.uint8),
            (st.segments, st.tri_tests, st.traces, st.accumulates))


@functools.lru_cache(maxsize=None)
def loop_reference(scene, size, spp, bounces, variant, mode, partition, first, n, clear=False, env=None):
    """The per-frame loop on a context with the option off, the displayed accumulator read back around every
    fold: ([(frame, changed, sum, max)], accumulator, trace image, counters) -- after an optional clear
    (init trace + accumulate(0), as RayTracingApp.open does) whose record comes first."""
    case = SceneCase(scene, size, spp, bounces)
    if env is not None:
        case.settings.use_environment_lighting = env
    ctx = case.context(mode=mode, variant=variant, partition=partition)
    if seeded(size, partition):
        seed_accumulator(ctx, size, mode)
    real = ctx.global_rows() < ctx.height
    recs = []

    def fold(k):
        before = ctx.read(_lib.IMG_ACCUM)[real]
        ctx.accumulate(k)
        recs.append((k,) + fold_ref.records(before, ctx.read(_lib.IMG_ACCUM)[real]))

    if clear:
        ctx.trace(case.push(init=True))
        fold(0)
    for k in range(first, first + n):
        ctx.trace(case.push(k))
        fold(k)
    out = (tuple(recs),) + state(ctx, mode)
    ctx.close()
    return out


CASES = [
    ("island", (96, 64), 3, 9, RGBA8, None),
    ("island", (96, 64), 3, 8, RGBA32F, None),
    ("box", (45, 33), 3, 5, RGBA8, None),              # not persistent; 1,485 pixels, no multiple of 64
    ("island", (80, 70), 2, 9, RGBA8, (8, 2, 3)),      # part 2: global rows up to 71, 2 of 24 local rows are padding
    ("box", (1, 1), 2, 0, RGBA8, None),
    ("box", (300, 1), 2, 0, RGBA32F, None),
]


@pytest.mark.parametrize("fpl", [1, 3, 16])
@pytest.mark.parametrize("scene,size,spp,variant,mode,partition", CASES)
def test_records_of_compute_n(scene, size, spp, variant, mode, partition, fpl):
    """7 frames from rng_offset 3 through hrt_compute_n with the option on (launches of 1, 3 + 2 + 2 or 7
    frames): one record per frame in fold order, equal to the reference's; total 7; accumulator, trace
    image and counters those of the option-off loop.  At fpl 1 the per-frame hrt_trace / hrt_accumulate loop
    with the option on as well."""
    first, n = 3, 7
    want, acc, trace, counters = loop_reference(scene, size, spp, 8, variant, mode, partition, first, n)
    assert any(r[1] for r in want)  # the case folds something
    case = SceneCase(scene, size, spp, 8)
    for per_frame in ([False, True] if fpl == 1 else [False]):
        ctx = case.context(mode=mode, variant=variant, partition=partition,
                           options={_lib.OPT_FRAMES_PER_LAUNCH: fpl, _lib.OPT_FOLD_RECORDS: 1})
        if seeded(size, partition):
            seed_accumulator(ctx, size, mode)
        if per_frame:
            for k in range(first, first + n):
                ctx.trace(case.push(k))
                ctx.accumulate(k)
        else:
            ctx.compute_n(case.push(first), n)
        recs, total = ctx.fold_records(with_total=True)
        got = state(ctx, mode)
        ctx.close()
        assert rec_tuples(recs) == list(want)
        assert total == n
        assert np.array_equal(got[0], acc) and np.array_equal(got[1], trace)
        assert got[2] == counters


def test_padding_rows_change_but_are_not_counted():
    """The partition case: part 2 of (8, 2, 3) on 80x70 holds 24 local rows of which the last 2 (global rows
    70, 71) are padding.  Its seeded accumulator makes a fold change pixels of those rows too; the record
    counts the 22 real rows only."""
    case = SceneCase("island", (80, 70), 2, 8)
    ctx = case.context(variant=9, partition=(8, 2, 3), options={_lib.OPT_FOLD_RECORDS: 1})
    rows = ctx.global_rows()
    assert len(rows) == 24 and int((rows < 70).sum()) == 22 and (rows[:22] < 70).all()
    seed_accumulator(ctx, (80, 70), RGBA8)
    ctx.trace(case.push(3))
    before = ctx.read(_lib.IMG_ACCUM)
    ctx.accumulate(3)
    after = ctx.read(_lib.IMG_ACCUM)
    got = rec_tuples(ctx.fold_records())
    ctx.close()
    assert (before[22:] != after[22:]).any()
    assert got == [(3,) + fold_ref.records(before[:22], after[:22])]
    assert got[0][1:] != fold_ref.records(before, after)


def test_first_records_match_the_oracle():
    """Island 96x64, 3 spp, 8 bounces: the clear's record (a fresh accumulator already holds the cleared
    state: zeros) and the records of frames 1..4 against the CPU oracle's trace and combiner alone."""
    want = fold_ref.oracle_records("island", (96, 64), 3, 8, 4)
    case = SceneCase("island", (96, 64), 3, 8)
    ctx = case.context(options={_lib.OPT_FOLD_RECORDS: 1})
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    ctx.compute_n(case.push(1), 4)
    got = rec_tuples(ctx.fold_records())
    ctx.close()
    assert got == [(0, 0, 0, 0)] + [(k + 1,) + want[k] for k in range(4)]


@pytest.mark.parametrize("mode", [RGBA8, RGBA32F])
def test_accumulate_present_records(mode):
    """hrt_accumulate_present with the option on (its two-pass path): the target bytes, the ticket and the
    records of hrt_accumulate + hrt_present on a twin with the option on, whose records are the reference's."""
    size, first, n = (64, 48), 1, 3
    want, acc, _, _ = loop_reference("box", size, 2, 4, 0, mode, None, first, n, clear=True)
    case = SceneCase("box", size, 2, 4)
    targets, tickets, recs, accs = [], [], [], []
    for fused_call in (True, False):
        ctx = case.context(mode=mode, options={_lib.OPT_FOLD_RECORDS: 1})
        t = Target(size[0], size[1])
        ctx.trace(case.push(init=True))
        ctx.accumulate(0)
        tk = []
        for k in range(first, first + n):
            ctx.trace(case.push(k))
            if fused_call:
                tk.append(ctx.accumulate_present(k, *t.args(), fmt=BGRA))
            else:
                ctx.accumulate(k)
                tk.append(ctx.present(_lib.IMG_ACCUM, *t.args(), fmt=BGRA))
        ctx.present_wait(tk[-1])
        assert all(ctx.present_done(x) for x in tk)
        assert ctx.stats().accumulates == n + 1
        t.expect(ctx.read(_lib.IMG_ACCUM), BGRA)
        targets.append(t.buf.read())
        tickets.append(tk)
        recs.append(rec_tuples(ctx.fold_records()))
        accs.append(ctx.read(_lib.IMG_ACCUM, native(mode)).view(np.uint8))
        t.free()
        ctx.close()
    assert tickets[0] == tickets[1] == [1, 2, 3]
    assert np.array_equal(targets[0], targets[1])
    assert recs[0] == recs[1] == list(want)
    assert np.array_equal(accs[0], acc) and np.array_equal(accs[1], acc)


def test_deferred_combines_record_in_frame_order():
    """HRT_OPT_DEFER_COMBINE = 1: the folds run at the flush, several frames per pass; hrt_get_fold_records
    flushes and returns the same records in frame order."""
    first, n = 3, 7
    want, acc, trace, counters = loop_reference("island", (96, 64), 3, 8, 9, RGBA8, None, first, n)
    case = SceneCase("island", (96, 64), 3, 8)
    ctx = case.context(variant=9, options={_lib.OPT_DEFER_COMBINE: 1, _lib.OPT_FOLD_RECORDS: 1})
    for k in range(first, first + n):
        ctx.trace(case.push(k))
        ctx.accumulate(k)
    recs, total = ctx.fold_records(with_total=True)
    got = state(ctx, RGBA8)
    ctx.close()
    assert rec_tuples(recs) == list(want) and total == n
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], trace) and got[2] == counters


def test_ring_wrap():
    """Box 16x16: 1,020 hrt_accumulate calls of one traced image with rising frame numbers, then hrt_compute_n
    of 16 frames in one launch, whose fold straddles the ring's end (slots 1020..1023, 0..11).  total is 1,036,
    the 1,024 newest records are the expected ones, and setting the option again empties the ring."""
    size, ring = (16, 16), _lib.FOLD_RECORD_RING
    case = SceneCase("box", size, 2, 4)
    ref = case.context(variant=9)
    ctx = case.context(variant=9, options={_lib.OPT_FRAMES_PER_LAUNCH: 16, _lib.OPT_FOLD_RECORDS: 1})
    for c in (ref, ctx):
        seed_accumulator(c, size, RGBA8)
        c.trace(case.push(1))
    # the reference: the oracle's combiner from the context's own read-backs, checked against the context's
    # accumulator at the end (the combiner itself is pinned by tests/test_gpu_parity.py)
    import pyoracle
    acc, img = ref.read(_lib.IMG_ACCUM), ref.read(_lib.IMG_TRACE)
    want = []
    for k in range(1, 1021):
        before = acc.copy()
        pyoracle.accumulate_rgba8(k, acc, img)
        want.append((k,) + fold_ref.records(before, acc))
        ref.accumulate(k)
        ctx.accumulate(k)
    assert np.array_equal(ref.read(_lib.IMG_ACCUM), acc)
    for k in range(1021, 1037):
        ref.trace(case.push(k))
        before = ref.read(_lib.IMG_ACCUM)
        ref.accumulate(k)
        want.append((k,) + fold_ref.records(before, ref.read(_lib.IMG_ACCUM)))
    ctx.compute_n(case.push(1021), 16)
    assert ctx.stats().last_frames == 16  # one launch: the multi-frame fold straddled the ring's end
    recs, total = ctx.fold_records(with_total=True)
    assert total == 1036 and len(recs) == ring
    assert rec_tuples(recs) == want[-ring:]
    assert any(r[1] for r in want[:8]) and rec_tuples(ctx.fold_records(cap=5)) == want[-5:]
    assert np.array_equal(ctx.read(_lib.IMG_ACCUM), ref.read(_lib.IMG_ACCUM))
    ctx.set_option(_lib.OPT_FOLD_RECORDS, 1)
    recs, total = ctx.fold_records(with_total=True)
    assert len(recs) == 0 and total == 0
    ctx.accumulate(1037)
    recs, total = ctx.fold_records(with_total=True)
    assert total == 1 and int(recs[0]["frame"]) == 1037
    ctx.set_option(_lib.OPT_FOLD_RECORDS, 0)
    ctx.accumulate(1038)
    recs, total = ctx.fold_records(with_total=True)
    assert len(recs) == 0 and total == 0
    ref.close()
    ctx.close()


def test_frozen_accumulator():
    """RGBA8: a fold at frame HRT_RGBA8_FREEZE_FRAME and at frame 4000 changes no pixel of any accumulator,
    whatever the traced frame holds: all-zero records, the accumulator unchanged."""
    size = (45, 33)
    case = SceneCase("box", size, 2, 4)
    ctx = case.context(options={_lib.OPT_FOLD_RECORDS: 1})
    acc = np.random.default_rng(7).integers(0, 256, (size[1], size[0], 4), dtype=np.uint8)
    acc[..., 3] = 255
    ctx.load_accumulator(acc)
    ctx.trace(case.push(1))
    assert ctx.read(_lib.IMG_TRACE)[..., :3].any()
    ctx.accumulate(_lib.RGBA8_FREEZE_FRAME)
    ctx.accumulate(4000)
    got = rec_tuples(ctx.fold_records())
    after = ctx.read(_lib.IMG_ACCUM)
    ctx.accumulate(_lib.RGBA8_FREEZE_FRAME - 300)  # (not frozen yet: the same fold does change pixels)
    live = rec_tuples(ctx.fold_records())[-1]
    ctx.close()
    assert got == [(_lib.RGBA8_FREEZE_FRAME, 0, 0, 0), (4000, 0, 0, 0)]
    assert np.array_equal(after, acc)
    assert live[1] > 0


def test_guard_bands():
    """The debug library's guard bands around every device buffer (the ring and the count pass's scratch ring
    included) stay intact through recorded folds, a wrapped ring and hrt_compute_until."""
    case = SceneCase("box", (45, 33), 2, 4)
    ctx = case.context(variant=9, debug=True, options={_lib.OPT_FRAMES_PER_LAUNCH: 16, _lib.OPT_FOLD_RECORDS: 1})
    ctx.trace(case.push(1))
    for k in range(1, 1018):
        ctx.accumulate(k)
    ctx.compute_n(case.push(1018), 16)
    done, _ = ctx.compute_until(case.push(1), 20, max_delta=40, quiet_frames=2)
    assert done >= 2
    assert ctx.fold_records(with_total=True)[1] == 1017 + 16 + done
    n, bad = ctx.check_guards()
    ctx.close()
    assert n > 0 and bad == 0


# ---- hrt_compute_until ----------------------------------------------------------------------------------

UNTIL = [
    ("island", (96, 64), 3, 8, 0, (1000, ANY, 2), 23),
    ("island", (96, 64), 3, 8, 0, (ANY, 12, 3), 18),
    ("box", (45, 33), 3, 8, 5, (ANY, 20, 2), 13),   # not persistent: one frame per launch
]
MAX_FRAMES = 40


@functools.lru_cache(maxsize=None)
def compute_n_reference(scene, size, spp, bounces, variant, n, env=None):
    """hrt_compute_n(pc from frame 1, n) after the clear on a fresh context: accumulator, trace image, counters."""
    case = SceneCase(scene, size, spp, bounces)
    if env is not None:
        case.settings.use_environment_lighting = env
    ctx = case.context(variant=variant)
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    if n:
        ctx.compute_n(case.push(1), n)
    out = state(ctx, RGBA8)
    ctx.close()
    return out


@pytest.mark.parametrize("records_on", [0, 1])
@pytest.mark.parametrize("fpl", [1, 3, 16])
@pytest.mark.parametrize("scene,size,spp,bounces,variant,rule,oracle_stop", UNTIL)
def test_compute_until_stops_where_the_reference_does(scene, size, spp, bounces, variant, rule, oracle_stop, fpl,
                                                      records_on):
    """From frame 1 after a clear, at most 40 frames: the stop is the reference context's (strictly inside
    the call, and the frame the CPU oracle alone gives), the accumulator and the trace image are those of
    hrt_compute_n(pc, s) on a fresh context, accumulates advanced by s, at least s frames were traced, and the
    ring gained s records with the option on and none with it off."""
    want = loop_reference(scene, size, spp, bounces, variant, RGBA8, None, 1, MAX_FRAMES, clear=True)[0]
    frames = [r[1:] for r in want[1:]]  # (changed, sum, max) of frames 1..40
    s, settled = fold_ref.stop_frame(frames, MAX_FRAMES, *rule)
    assert settled and 1 < s < MAX_FRAMES and s == oracle_stop
    acc, trace, counters = compute_n_reference(scene, size, spp, bounces, variant, s)
    case = SceneCase(scene, size, spp, bounces)
    ctx = case.context(variant=variant, options={_lib.OPT_FRAMES_PER_LAUNCH: fpl, _lib.OPT_FOLD_RECORDS: records_on})
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    before = ctx.stats()
    total0 = ctx.fold_records(with_total=True)[1]
    done, ok = ctx.compute_until(case.push(1), MAX_FRAMES, *rule)
    recs, total = ctx.fold_records(with_total=True)
    got = state(ctx, RGBA8)
    ctx.close()
    assert (done, ok) == (s, True)
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], trace)
    assert got[2][3] - before.accumulates == s and got[2][3] == counters[3]
    assert got[2][2] - before.traces >= s
    if records_on:
        assert total - total0 == s and total0 == 1
        assert rec_tuples(recs) == list(want[:s + 1])
    else:
        assert total == total0 == 0 and len(recs) == 0


@pytest.mark.parametrize("fpl", [1, 4])
def test_rule_that_cannot_be_met(fpl):
    """No frame of the lit island leaves every pixel unchanged: frames_done == max_frames, not settled, the
    bytes of hrt_compute_n(pc, max_frames)."""
    n = 6
    acc, trace, counters = compute_n_reference("island", (96, 64), 3, 8, 0, n)
    case = SceneCase("island", (96, 64), 3, 8)
    ctx = case.context(options={_lib.OPT_FRAMES_PER_LAUNCH: fpl})
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    done, ok = ctx.compute_until(case.push(1), n, max_changed_pixels=0, max_delta=0, quiet_frames=1)
    got = state(ctx, RGBA8)
    assert ctx.compute_until(case.push(1), 0) == (0, False)  # max_frames == 0: nothing happens
    assert state(ctx, RGBA8)[2] == got[2]
    ctx.close()
    assert (done, ok) == (n, False)
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], trace) and got[2] == counters


@pytest.mark.parametrize("fpl,quiet_frames", [(1, 3), (16, 3), (2, 5)])
def test_black_scene_settles_at_once(fpl, quiet_frames):
    """Island with the environment light off after a clear: every frame is black, every record zero, so the
    call stops after exactly quiet_frames frames."""
    acc, trace, _ = compute_n_reference("island", (96, 64), 3, 8, 0, quiet_frames, env=False)
    assert not acc.reshape(-1, 4)[:, :3].any()
    case = SceneCase("island", (96, 64), 3, 8)
    case.settings.use_environment_lighting = False
    ctx = case.context(options={_lib.OPT_FRAMES_PER_LAUNCH: fpl, _lib.OPT_FOLD_RECORDS: 1})
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    done, ok = ctx.compute_until(case.push(1), 30, max_changed_pixels=0, max_delta=0, quiet_frames=quiet_frames)
    recs = rec_tuples(ctx.fold_records())
    got = state(ctx, RGBA8)
    ctx.close()
    assert (done, ok) == (quiet_frames, True)
    assert recs == [(k, 0, 0, 0) for k in range(quiet_frames + 1)]
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], trace)


def test_rejected_arguments():
    """Each rejected argument returns HRT_ERR_INVALID_ARGUMENT with a message naming the reason, before
    anything is enqueued: counters, ring and images are untouched, and a following hrt_compute_n matches the
    per-frame loop."""
    first, n = 3, 7
    want, acc, trace, counters = loop_reference("island", (96, 64), 3, 8, 9, RGBA8, None, first, n)
    case = SceneCase("island", (96, 64), 3, 8)
    ctx = case.context(variant=9, options={_lib.OPT_FOLD_RECORDS: 1})
    lib, h = ctx.lib, ctx.handle
    pc, init_pc = case.push(first), case.push(first, init=True)
    done, settled = ctypes.c_uint32(77), ctypes.c_uint32(77)

    def call(pc=pc, rule=_lib.SettleRule(0, 0, 1, 0), done_ref=ctypes.byref(done)):
        st = lib.hrt_compute_until(h, ctypes.byref(pc), 5, None if rule is None else ctypes.byref(rule), done_ref,
                                   ctypes.byref(settled))
        return st, lib.hrt_last_error(h).decode()

    for kwargs, reason in [({"rule": None}, "NULL"), ({"done_ref": None}, "NULL"),
                           ({"rule": _lib.SettleRule(0, 0, 1, 1)}, "flags"),
                           ({"rule": _lib.SettleRule(0, 0, 0, 0)}, "quiet_frames"),
                           ({"pc": init_pc}, "init")]:
        st, msg = call(**kwargs)
        assert st == 1 and "hrt_compute_until" in msg and reason in msg, (kwargs, st, msg)
    assert (done.value, settled.value) == (77, 77)
    # settled may be NULL
    rule = _lib.SettleRule(ANY, ANY, 1, 0)
    assert lib.hrt_compute_until(h, ctypes.byref(pc), 0, ctypes.byref(rule), ctypes.byref(done), None) == 0
    assert done.value == 0
    st = ctx.stats()
    assert (st.traces, st.accumulates) == (0, 0) and ctx.fold_records(with_total=True)[1] == 0
    ctx.compute_n(pc, n)
    recs = rec_tuples(ctx.fold_records())
    got = state(ctx, RGBA8)
    ctx.close()
    assert recs == list(want)
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], trace) and got[2] == counters


def test_rejected_contexts():
    """A context of a row-tile partition and a context joined to a communicator are rejected (the parts
    would stop at different frames); the message names the reason and nothing runs."""
    case = SceneCase("box", (40, 32), 2, 4)
    part = case.context(partition=(8, 0, 2))
    with pytest.raises(_lib.HrtError, match="partition"):
        part.compute_until(case.push(1), 4, quiet_frames=1)
    assert part.stats().traces == 0
    part.close()
    group = [case.context(partition=(8, i, 2)) for i in range(2)]  # one device: joined by device copies
    HrtContext.comm_init_all(group)
    assert group[0].comm_info()[2] == _lib.COMM_DEVICE_COPY
    for member in group:
        with pytest.raises(_lib.HrtError, match="communicator"):
            member.compute_until(case.push(1), 4, quiet_frames=1)
        assert member.stats().traces == 0
    for member in group:
        member.close()


# ---- mirrors ----------------------------------------------------------------------------------------------

def test_python_compute_until_then_render():
    """compute_until_then_render: app.frame advances by frames_done, the render hook runs once, and the
    accumulator is the one of compute_n_then_render(frames_done)."""
    size, rule = (45, 33), dict(max_delta=20, quiet_frames=2)
    renders = []
    cam, settings = E.preset("box")
    settings.num_samples, settings.max_bounces = 3, 8
    app = E.RayTracingApp(cam, settings, device=0)
    app.open(size)
    app.pipeline = app.pipeline[:2] + (lambda image: renders.append(image.read()),)
    done, settled = E.compute_until_then_render(app, 40, **rule)
    assert settled and done == 13 and app.frame == 1 + done and len(renders) == 1
    cam, settings = E.preset("box")
    settings.num_samples, settings.max_bounces = 3, 8
    twin = E.RayTracingApp(cam, settings, device=0)
    twin.open(size)
    E.compute_n_then_render(twin, done)
    assert np.array_equal(renders[0], twin.context.read(_lib.IMG_ACCUM))
    app.close()
    twin.close()


CPP_PROGRAM = r"""
#include <cstdio>
#include "hrt_app.hpp"
// box-like scene of the C++ mirror's own records: two spheres under the environment light
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    epq::RayTracerSettings s;
    s.num_samples = 3;
    s.max_bounces = 4;
    s.use_environment_lighting = true;
    s.sphere_data = {epq::Sphere{{0.0f, -100.5f, -1.0f}, 100.0f, epq::LambertianMaterial{{0.8f, 0.8f, 0.0f}}},
                     epq::Sphere{{0.0f, 0.0f, -1.2f}, 0.5f, epq::LambertianMaterial{{0.7f, 0.3f, 0.3f}}}};
    epq::Camera cam;
    cam.position = {0.0f, 0.3f, 1.5f};
    cam.direction = {0.0f, -0.1f, -1.0f};
    const hrt_settle_rule rule{0xFFFFFFFFu, 20u, 2u, 0u};
    int renders = 0;
    epq::RayTracingApp app(cam, s, 0);
    app.open({45u, 33u}, [&](const epq::Image&) { ++renders; });
    app.context().set_option(HRT_OPT_FOLD_RECORDS, 1);
    const std::pair<uint32_t, bool> r = epq::compute_until_then_render(app, 40, rule);
    uint64_t total = 0;
    const std::vector<hrt_fold_record> recs = app.context().fold_records(HRT_FOLD_RECORD_RING, &total);
    const std::vector<uint8_t> a = app.context().read_rgba8(HRT_IMG_ACCUM);
    // the twin: hrt_compute_n of the same number of frames
    epq::RayTracingApp twin(cam, s, 0);
    twin.open({45u, 33u});
    epq::compute_n_then_render(twin, r.first);
    const bool same = a == twin.context().read_rgba8(HRT_IMG_ACCUM);
    uint32_t quiet_tail = 0;
    for (size_t i = recs.size(); i-- > 0 && recs[i].max_delta <= 20u;) ++quiet_tail;
    std::FILE* f = std::fopen(argv[1], "w");
    std::fprintf(f, "%u %d %u %d %llu %zu %u %d %u\n", r.first, (int)r.second, app.frame(), renders,
                 (unsigned long long)total, recs.size(), recs.empty() ? 0u : recs.back().frame, (int)same, quiet_tail);
    std::fclose(f);
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 10;
  }
  return 0;
}
"""


def test_cpp_compute_until_then_render(tmp_path):
    """include/hrt_app.hpp: Context::compute_until / fold_records and compute_until_then_render, in a program
    compiled here against the in-tree library."""
    src, exe, out = tmp_path / "until.cpp", tmp_path / "until", tmp_path / "until.txt"
    src.write_text(CPP_PROGRAM)
    libdir = os.path.join(ROOT, "epq_raytracer_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", libdir, "-lhip_raytrace", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    done, settled, frame, renders, total, nrecs, last_frame, same, quiet_tail = (int(v) for v in out.read_text().split())
    assert settled == 1 and 2 <= done < 40
    assert frame == 1 + done and renders == 2  # open's present and the one after the call
    assert total == nrecs == done and last_frame == done
    assert same == 1 and quiet_tail == 2  # stopped at the FIRST run of two quiet frames
