"""The image passes of hrt_image.hip enumerated on the device: the combiner (accumulate), the multi-frame
fold (accumulate_frames), the recording folds (fold_records, storing and counting), the fused fold and
present (accumulate_present), the two format converters, and pack_rgba8 / unorm8 inside the present kernels.

Every expected value comes from tests/image_ref.py, a numpy float32 restatement that tests/test_image_ref.py
pins to the CPU oracle.  Every comparison is exact: bytes, or 32-bit patterns with one rule -- two NaNs are
equal whatever their sign and payload, because the host and the device generate different default NaNs and
S1 does not pin them (image_ref.same_floats).

Inputs, through the public API only.  The trace image is rendered: 256 small light spheres on an arc, sphere
j on the ray of column x = j, caller-supplied ray centres (the same for every row), no jitter, one sample, no
bounce, no environment light -- so every pixel of column x shows sphere x's emission whatever rng_offset is.
It is compared with the oracle's frame once (kernel variant AUTO) and its read-back is the reference's input
from then on.  The accumulator is loaded (hrt_load_accumulator).
  RGBA8: emission (x, (37 x + 11) mod 256, 255 - x) / 255 and accumulator row y = (y, (91 y + 5) mod 256,
    255 - y, (3 y) mod 256): at 256 x 256 every (accumulator byte, trace byte) pair occurs in every colour
    channel.
  RGBA32F: the emissions are the first 256 values of image_ref.float_pool() (the specials, then the UNORM8
    rounding ties and their neighbours) under the same three column maps, and the 256 x 258 accumulator
    holds the whole pool in all four channels: every pool value meets at least 16 different trace values.
Each case asserts that premise on the bytes it read back before it compares anything."""
import functools

import numpy as np
import pytest

import fold_ref
import image_ref
from epq_raytracer_amd import _lib
from epq_raytracer_amd.pipeline import RayTracerSettings
from epq_raytracer_amd.scene import Camera, LightMaterial, Sphere
from helpers import SceneCase
from test_gpu_present import BGRA, RGBA, Target

pytestmark = pytest.mark.gpu

RGBA8, RGBA32F = _lib.MODE_RGBA8, _lib.MODE_RGBA32F
F_ALL, F_SOME = image_ref.F_ALL, image_ref.F_SOME
STARTS = (1, 500, 2**24 - 8, 2**32 - 3)  # runs of 16 consecutive frames; the last one wraps through frame 0
RUN = 16
F_FLOAT = (0, 1, 2, 3, 255, 2**24 + 1, 2**32 - 2, 2**32 - 1)
M32 = 0xFFFFFFFF
# hrt_compute_n / hrt_compute_until trace several frames per launch with the persistent kernels only, and AUTO
# gives this mesh-less scene BUNDLE (one frame per launch): the cases that must fold a stack ask for
# BUNDLE_CULL_LDS, which runs any scene, and assert hrt_stats.last_frames.
BATCHING = 7


class Columns(SceneCase):
    """The sphere scene: emissions[j] (3 float32) is sphere j's light, seen by every pixel of column j."""

    def __init__(self, size, emissions):
        w, h = size
        spheres = []
        for j in range(256):
            d = np.array([1.0, 0.0, (j - 127.5) / 128])
            spheres.append(Sphere(10 * d / np.linalg.norm(d), 0.02, LightMaterial(list(emissions[j]) + [1.0])))
        settings = RayTracerSettings(1, 0, False, sample_jitter=0.0, sphere_data=spheres)
        super().__init__(None, size, 1, 0, settings=settings, camera=Camera())
        centres = np.zeros((h, w, 4), np.float32)
        centres[..., 0] = 1.0
        centres[..., 2] = ((np.arange(w) - 127.5) / 128)[None, :]
        self.rays = np.zeros(w * h, dtype=_lib.RAY_DTYPE)
        self.rays["sample_centre"] = centres.reshape(-1, 4)
        self.n_rays, self.jitter = w * h, 0.0

    def push(self, rng_offset=None, init=False):
        pc = super().push(rng_offset, init)
        pc.cam_pos[:] = [0.0, 0.0, 0.0, 1.0]
        pc.cam_alignment_mat[:] = [float(v) for v in np.eye(4, dtype=np.float32).reshape(-1)]
        return pc


def byte_case(size=(256, 256)):
    return Columns(size, image_ref.unorm8_to_float(image_ref.column_bytes()))


def float_emissions():
    return image_ref.float_pool()[image_ref.column_bytes().astype(np.int64)]


def traced(case, mode=RGBA8, debug=False, options=None, offset=1, variant=0):
    ctx = case.context(mode=mode, debug=debug, options=options, variant=variant)
    ctx.trace(case.push(offset))
    return ctx


def deferred_run(case, acc, start, mode=RGBA8, records=0):
    """A FRESH context with HRT_OPT_DEFER_COMBINE = 1, the accumulator loaded, then RUN x (trace, accumulate) of
    the frames from start: the context's first 16 deferred traces take ring slots 0..15, consecutive slots and
    frames, so the flush folds them as ONE run of 16 (a context that has traced before starts at slot 1 and
    folds 15 + 1).  The library reports no count of fold passes, so this is by construction, not asserted.
    Returns the context and the accumulator read back before the run (the premise's first half)."""
    ctx = case.context(mode=mode, options={_lib.OPT_DEFER_COMBINE: 1, _lib.OPT_FOLD_RECORDS: records})
    ctx.load_accumulator(acc)
    loaded = ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA8 if mode == RGBA8 else _lib.FMT_RGBA32F)
    assert ctx.stats().traces == 0
    for k in range(RUN):
        ctx.trace(case.push((start + k) & M32))
        ctx.accumulate((start + k) & M32)
    return ctx, loaded


@functools.lru_cache(maxsize=None)
def byte_inputs(size=(256, 256)):
    """(case, accumulator to load, the device's trace image): the trace image equals the oracle's frame and
    does not depend on rng_offset (every offset the runs below use is traced and read once)."""
    case = byte_case(size)
    acc, _ = image_ref.pairs_images(*size)
    ctx = traced(case)
    trace = ctx.read(_lib.IMG_TRACE)
    assert np.array_equal(trace, case.oracle(1)[0])
    if size == (256, 256):
        for start in STARTS:
            for k in range(RUN):
                ctx.trace(case.push((start + k) & M32))
                assert np.array_equal(ctx.read(_lib.IMG_TRACE), trace), (start, k)
    ctx.close()
    trace.setflags(write=False)
    acc.setflags(write=False)
    return case, acc, trace


def check_pairs(ctx, acc, trace):
    """The premise, on the bytes the context holds."""
    got_acc, got_trace = ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_TRACE)
    assert np.array_equal(got_acc, acc) and np.array_equal(got_trace, trace)
    image_ref.assert_all_pairs(got_acc, got_trace)


@functools.lru_cache(maxsize=None)
def byte_chain(size, start, n):
    """The accumulators after each of the n folds of frames start, start + 1, ... (mod 2^32) from the loaded
    one, and the fold records: ([accumulator], [(frame, changed, sum, max)])."""
    _, acc, trace = byte_inputs(size)
    fold = image_ref.fold_rgba8_by_pairs if size == (256, 256) else image_ref.fold_rgba8
    accs, recs, cur = [], [], acc
    for k in range(n):
        frame = (start + k) & M32
        nxt = fold(frame, cur, trace)
        recs.append((frame,) + image_ref.record(cur, nxt))
        accs.append(nxt)
        cur = nxt
    return accs, recs


def rec_tuples(recs):
    assert not recs["reserved"].any()
    return [(int(r["frame"]), int(r["changed_pixels"]), int(r["abs_delta_sum"]), int(r["max_delta"])) for r in recs]


def first_diff(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} bytes differ, first at (y, x, ch) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


# ---- RGBA8 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part", range(4))
def test_accumulate_every_pair_every_frame(part):
    """hrt_accumulate (accumulate<uint32_t>, combine_rgba8_fast: the LDS table of k / 255, the shared
    reciprocal of frame + 1, Markstein's one-correction quotient) on all 65,536 channel pairs at every frame
    of F_ALL, in four slices of it: byte for byte image_ref.fold_rgba8.  And what HRT_RGBA8_FREEZE_FRAME
    claims, on the device's bytes: some colour byte changes at frame 509, none at any frame of 510..1199."""
    case, acc, trace = byte_inputs()
    frames = F_ALL[part::4]
    ctx = traced(case)
    ctx.load_accumulator(acc)
    check_pairs(ctx, acc, trace)
    for frame in frames:
        ctx.load_accumulator(acc)
        ctx.accumulate(frame)
        got = ctx.read(_lib.IMG_ACCUM)
        want = image_ref.fold_rgba8_by_pairs(frame, acc, trace)
        assert np.array_equal(got, want), f"frame {frame}: {first_diff(got, want)}"
        changed = bool((got[..., :3] != acc[..., :3]).any())
        if frame == _lib.RGBA8_FREEZE_FRAME - 1:
            assert changed
        if _lib.RGBA8_FREEZE_FRAME <= frame < 1200:
            assert not changed, frame
    ctx.close()


def test_accumulate_present_every_pair():
    """hrt_accumulate_present at the image's own size (the fused kernel) on F_SOME: the accumulator as above,
    the target present_ref's flip (and swap) of it in both formats and with a pitch wider than the row, whose
    padding keeps its sentinel."""
    case, acc, trace = byte_inputs()
    ctx = traced(case)
    ctx.load_accumulator(acc)
    check_pairs(ctx, acc, trace)
    targets = [(Target(256, 256, 256 * 4 + 16), BGRA), (Target(256, 256, 256 * 4 + 16), RGBA), (Target(256, 256), BGRA)]
    for frame in F_SOME:
        want = image_ref.fold_rgba8(frame, acc, trace)
        for t, fmt in targets:
            t.buf.fill()
            ctx.load_accumulator(acc)
            ctx.present_wait(ctx.accumulate_present(frame, *t.args(), fmt=fmt))
            got = ctx.read(_lib.IMG_ACCUM)
            assert np.array_equal(got, want), f"frame {frame}: {first_diff(got, want)}"
            t.expect(want, fmt)
    ctx.close()
    for t, _ in targets:
        t.free()


@pytest.mark.parametrize("start", STARTS)
def test_runs_of_frames_every_pair(start):
    """16 consecutive frames folded in one pass (accumulate_frames<uint32_t>, nf = 16): deferred trace +
    accumulate calls on a fresh context (deferred_run), and hrt_compute_n as one launch of 16 frames
    (last_frames asserted); one read each, against the chain of image_ref.fold_rgba8.  The start 2^32 - 3
    runs ..., 2^32 - 1, 0, 1, ...: the wrap folds a clear in mid-run."""
    case, acc, trace = byte_inputs()
    want = byte_chain((256, 256), start, RUN)[0][-1]
    ctx, loaded = deferred_run(case, acc, start)
    got, got_trace = ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_TRACE)
    ctx.close()
    assert np.array_equal(loaded, acc) and np.array_equal(got_trace, trace)
    image_ref.assert_all_pairs(loaded, got_trace)
    assert np.array_equal(got, want), f"deferred run from {start}: {first_diff(got, want)}"
    ctx = traced(case, options={_lib.OPT_FRAMES_PER_LAUNCH: RUN}, variant=BATCHING)
    ctx.load_accumulator(acc)
    check_pairs(ctx, acc, trace)
    ctx.compute_n(case.push(start), RUN)
    got, st = ctx.read(_lib.IMG_ACCUM), ctx.stats()
    assert np.array_equal(ctx.read(_lib.IMG_TRACE), trace)
    ctx.close()
    assert (st.last_kernel, st.last_frames) == (BATCHING, RUN)  # one launch: the stack kernel folded all 16
    assert np.array_equal(got, want), f"hrt_compute_n from {start}: {first_diff(got, want)}"


def test_fold_records_single_frames():
    """HRT_OPT_FOLD_RECORDS = 1, one frame per fold (fold_records<uint32_t, true>, nf = 1) on F_SOME: every
    record is image_ref.record of the reference fold, and the accumulator is the one without the option."""
    case, acc, trace = byte_inputs()
    ctx = traced(case, options={_lib.OPT_FOLD_RECORDS: 1})
    ctx.load_accumulator(acc)
    check_pairs(ctx, acc, trace)
    want_recs = []
    for frame in F_SOME:
        want = image_ref.fold_rgba8(frame, acc, trace)
        want_recs.append((frame,) + image_ref.record(acc, want))
        ctx.load_accumulator(acc)
        ctx.accumulate(frame)
        got = ctx.read(_lib.IMG_ACCUM)
        assert np.array_equal(got, want), f"frame {frame}: {first_diff(got, want)}"
    recs, total = ctx.fold_records(with_total=True)
    ctx.close()
    assert total == len(F_SOME) and rec_tuples(recs) == want_recs
    assert all(r[1] > 0 for r in want_recs)  # (the loaded alpha bytes become 255: every fold changes pixels)


@pytest.mark.parametrize("start", STARTS)
def test_fold_records_runs(start):
    """The same with 16 frames per fold (fold_records<uint32_t, true>, nf = 16): the deferred run on a fresh
    context and hrt_compute_n as one launch of 16 frames, with the option on."""
    case, acc, trace = byte_inputs()
    accs, want_recs = byte_chain((256, 256), start, RUN)
    for deferred in (True, False):
        if deferred:
            ctx, loaded = deferred_run(case, acc, start, records=1)
        else:
            ctx = traced(case, options={_lib.OPT_FOLD_RECORDS: 1, _lib.OPT_FRAMES_PER_LAUNCH: RUN}, variant=BATCHING)
            ctx.load_accumulator(acc)
            loaded = ctx.read(_lib.IMG_ACCUM)
            ctx.compute_n(case.push(start), RUN)
        recs, total = ctx.fold_records(with_total=True)
        got, got_trace, st = ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_TRACE), ctx.stats()
        ctx.close()
        assert np.array_equal(loaded, acc) and np.array_equal(got_trace, trace)
        image_ref.assert_all_pairs(loaded, got_trace)
        what = f"{'deferred run' if deferred else 'hrt_compute_n'} from {start}"
        if not deferred:
            assert (st.last_kernel, st.last_frames) == (BATCHING, RUN), what
        assert total == RUN and rec_tuples(recs) == want_recs, what
        assert np.array_equal(got, accs[-1]), f"{what}: {first_diff(got, accs[-1])}"


@pytest.mark.parametrize("fpl", [1, 16])
def test_compute_until_settles_where_the_chain_does(fpl):
    """hrt_compute_until (the counting fold, fold_records<uint32_t, false>) from the loaded accumulator at
    rng_offset 1 under (max_changed_pixels 0, quiet_frames 2), at most 600 frames: frames_done and settled
    are the reference chain's -- no later than frame 511, two frames into the freeze; the same frame folded
    again and again converges long before that -- and the accumulator
    is the chain's at that frame.  At HRT_OPT_FRAMES_PER_LAUNCH 16 the count pass runs with nf = 16 (the
    next-frame prefetch, a slot per frame, the stop in mid-launch); last_frames is asserted at both settings."""
    case, acc, trace = byte_inputs()
    accs, recs = byte_chain((256, 256), 1, _lib.RGBA8_FREEZE_FRAME + 1)
    s, settled = fold_ref.stop_frame([r[1:] for r in recs], 600, 0, fold_ref.ANY, 2)
    assert settled and 2 <= s <= _lib.RGBA8_FREEZE_FRAME + 1
    assert s % 16 != 0  # (the stop falls inside a launch of 16)
    ctx = traced(case, options={_lib.OPT_FRAMES_PER_LAUNCH: fpl}, variant=BATCHING)
    ctx.load_accumulator(acc)
    check_pairs(ctx, acc, trace)
    done, ok = ctx.compute_until(case.push(1), 600, max_changed_pixels=0, quiet_frames=2)
    got, st = ctx.read(_lib.IMG_ACCUM), ctx.stats()
    ctx.close()
    assert (st.last_kernel, st.last_frames) == (BATCHING, fpl)
    assert (done, ok) == (s, True)
    assert np.array_equal(got, accs[s - 1]), first_diff(got, accs[s - 1])


def test_rgba8_to_float_every_byte():
    """rgba8_to_f32: an RGBA8 accumulator holding all 256 bytes in all four channels read as
    HRT_FMT_RGBA32F is image_ref.unorm8_to_float of it, bitwise."""
    case, acc, _ = byte_inputs()
    ctx = case.context()
    ctx.load_accumulator(acc)
    got8, got = ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA32F)
    ctx.close()
    assert np.array_equal(got8, acc)
    for ch in range(4):
        assert len(np.unique(got8[..., ch])) == 256
    assert np.array_equal(got.view(np.uint32), image_ref.unorm8_to_float(acc).view(np.uint32))


def test_guard_bands_at_an_odd_size():
    """A 253 x 5 cut of the scene (1,265 pixels: no multiple of the workgroup) on the debug library: one
    hrt_accumulate, one deferred run and one records fold leave every guard band intact, and the bytes are
    the reference's."""
    size = (253, 5)
    case, acc, trace = byte_inputs(size)
    ctx = traced(case, debug=True)
    ctx.load_accumulator(acc)
    ctx.accumulate(3)
    got = ctx.read(_lib.IMG_ACCUM)
    assert np.array_equal(got, image_ref.fold_rgba8(3, acc, trace))
    for opts in ({_lib.OPT_DEFER_COMBINE: 1}, {_lib.OPT_DEFER_COMBINE: 1, _lib.OPT_FOLD_RECORDS: 1}):
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.load_accumulator(acc)
        for k in range(RUN):
            ctx.trace(case.push((2**32 - 3 + k) & M32))
            ctx.accumulate((2**32 - 3 + k) & M32)
        got = ctx.read(_lib.IMG_ACCUM)
        accs, recs = byte_chain(size, 2**32 - 3, RUN)
        assert np.array_equal(got, accs[-1])
    assert rec_tuples(ctx.fold_records()) == recs
    n, bad = ctx.check_guards()
    ctx.close()
    assert n > 0 and bad == 0


# ---- RGBA32F ----------------------------------------------------------------------------------------------

FSIZE = (256, 258)  # 8 pool values per row, each in 32 columns: ceil(2060 / 8) rows


def pool_image(size=FSIZE):
    """The accumulator to load: channel c of pixel (x, y) is pool[(8 y + x mod 8 + shift_c) mod 2060], alpha
    included, so pool value i sits in one row at 32 columns in every channel."""
    pool = image_ref.float_pool()
    w, h = size
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    base = 8 * y + x % 8
    return np.stack([pool[(base + s) % len(pool)] for s in (0, 701, 1402, 333)], -1)


@functools.lru_cache(maxsize=None)
def float_inputs():
    """(case, accumulator to load, the device's float trace image): the trace image equals the oracle's
    want_f32 frame (same_floats)."""
    case = Columns(FSIZE, float_emissions())
    ctx = traced(case, RGBA32F)
    trace = ctx.read(_lib.IMG_TRACE, _lib.FMT_RGBA32F)
    ctx.close()
    assert image_ref.same_floats(trace, case.oracle(1, want_f32=True)[1]).all()
    acc = pool_image()
    trace.setflags(write=False)
    acc.setflags(write=False)
    return case, acc, trace


def check_pool(ctx, acc, trace):
    """The premise, on what the context holds: the loaded pool image bit for bit, every pool pattern in every
    channel, and in each colour channel every pool value beside at least 16 different trace patterns."""
    check_pool_images(ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA32F), ctx.read(_lib.IMG_TRACE, _lib.FMT_RGBA32F), acc, trace)


def check_pool_images(got_acc, got_trace, acc, trace):
    assert np.array_equal(got_acc.view(np.uint32), acc.view(np.uint32))
    assert image_ref.same_floats(got_trace, trace).all()
    pool_bits = np.unique(image_ref.float_pool().view(np.uint32))
    for ch in range(4):
        assert np.array_equal(np.unique(got_acc[..., ch].view(np.uint32)), pool_bits)
    for ch in range(3):
        pairs = np.unique((got_acc[..., ch].view(np.uint32).astype(np.uint64) << np.uint64(32))
                          | got_trace[..., ch].view(np.uint32).astype(np.uint64))
        values, met = np.unique(pairs >> np.uint64(32), return_counts=True)
        assert np.array_equal(values, pool_bits.astype(np.uint64)) and met.min() >= 16, (ch, met.min())


def assert_same_floats(got, want, what):
    bad = np.argwhere(~image_ref.same_floats(got, want))
    assert len(bad) == 0, (f"{what}: {len(bad)} values differ, first at (y, x, ch) = {tuple(bad[0])}: "
                           f"{got.view(np.uint32)[tuple(bad[0])]:#010x} != {want.view(np.uint32)[tuple(bad[0])]:#010x}")


@functools.lru_cache(maxsize=None)
def float_chain(start, n):
    """(the accumulator after the n folds from frame start, [(frame, changed, sum, max)])."""
    _, acc, trace = float_inputs()
    cur, recs = acc, []
    for k in range(n):
        nxt = image_ref.fold_rgba32f((start + k) & M32, cur, trace)
        recs.append(((start + k) & M32,) + image_ref.record(cur, nxt))
        cur = nxt
    return cur, recs


def test_float_accumulate_and_present():
    """hrt_accumulate and hrt_accumulate_present (accumulate<float4>, accumulate_present<float4>) on the pool
    image at F_FLOAT against image_ref.fold_rgba32f; the fused kernel's target is image_ref.displayed of
    the result.  Float comparisons are on the 32-bit patterns, two NaNs being equal whatever their sign and
    payload (the host and the device generate different default NaNs; S1 does not pin them)."""
    case, acc, trace = float_inputs()
    ctx = traced(case, RGBA32F)
    ctx.load_accumulator(acc)
    check_pool(ctx, acc, trace)
    w, h = FSIZE
    targets = [(Target(w, h, w * 4 + 16), BGRA), (Target(w, h), RGBA)]
    for frame in F_FLOAT:
        want = image_ref.fold_rgba32f(frame, acc, trace)
        ctx.load_accumulator(acc)
        ctx.accumulate(frame)
        assert_same_floats(ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA32F), want, f"hrt_accumulate({frame})")
        for t, fmt in targets:
            t.buf.fill()
            ctx.load_accumulator(acc)
            ctx.present_wait(ctx.accumulate_present(frame, *t.args(), fmt=fmt))
            assert_same_floats(ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA32F), want, f"hrt_accumulate_present({frame})")
            t.expect(image_ref.displayed(want), fmt)
    ctx.close()
    for t, _ in targets:
        t.free()


@pytest.mark.parametrize("start", F_FLOAT)
def test_float_runs_of_frames(start):
    """16 deferred frames from each frame of F_FLOAT folded in one pass on a fresh context (deferred_run):
    accumulate_frames<float4>, and with HRT_OPT_FOLD_RECORDS = 1 fold_records<float4, true> with nf = 16,
    against the chain of image_ref.fold_rgba32f and its records, NaNs compared as above."""
    case, acc, trace = float_inputs()
    want, want_recs = float_chain(start, RUN)
    for records in (0, 1):
        ctx, loaded = deferred_run(case, acc, start, mode=RGBA32F, records=records)
        got, got_trace = ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA32F), ctx.read(_lib.IMG_TRACE, _lib.FMT_RGBA32F)
        recs = rec_tuples(ctx.fold_records()) if records else None
        ctx.close()
        check_pool_images(loaded, got_trace, acc, trace)
        assert_same_floats(got, want, f"deferred run from {start}, records {records}")
        assert recs is None or recs == want_recs, start


def test_float_pool_displayed():
    """pack_rgba8 / unorm8 on the whole pool, wherever the library shows a float image: hrt_read_image as
    HRT_FMT_RGBA8 (f32_to_rgba8), hrt_present at the image's size (the 128-bit row body; from a target 4
    bytes off the 16-byte grid the word path), scaled to (2 W, H / 2) (present_nearest), in both formats --
    all image_ref.displayed of the loaded image, byte for byte."""
    case, acc, trace = float_inputs()
    ctx = traced(case, RGBA32F)
    ctx.load_accumulator(acc)
    check_pool(ctx, acc, trace)
    want = image_ref.displayed(acc)
    assert len(np.unique(want)) == 256
    got = ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA8)
    assert np.array_equal(got, want), first_diff(got, want)
    w, h = FSIZE
    for t, fmt in [(Target(w, h), BGRA), (Target(w, h, w * 4 + 16), RGBA), (Target(w, h, offset=4), RGBA),
                   (Target(2 * w, h // 2), BGRA), (Target(2 * w, h // 2, 2 * w * 4 + 12), RGBA)]:
        ctx.present_wait(ctx.present(_lib.IMG_ACCUM, *t.args(), fmt=fmt))
        t.expect(want, fmt)
        t.free()
    ctx.close()


def test_float_pool_displayed_odd_width():
    """The same at an odd width (253 x 9 holds the pool once): rows that start off the 16-byte grid, and
    the last pixel of the others, go through present_rows' one-word tail."""
    size = (253, 9)
    pool = image_ref.float_pool()
    acc = pool[(np.arange(253 * 9 * 4) * 1031) % len(pool)].reshape(9, 253, 4)
    assert len(np.unique(acc.view(np.uint32))) == len(np.unique(pool.view(np.uint32)))
    case = Columns(size, float_emissions())
    ctx = case.context(mode=RGBA32F)
    ctx.load_accumulator(acc)
    assert np.array_equal(ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA32F).view(np.uint32), acc.view(np.uint32))
    want = image_ref.displayed(acc)
    got = ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA8)
    assert np.array_equal(got, want), first_diff(got, want)
    for t, fmt in [(Target(253, 9), BGRA), (Target(253, 9, 253 * 4 + 12), RGBA)]:
        ctx.present_wait(ctx.present(_lib.IMG_ACCUM, *t.args(), fmt=fmt))
        t.expect(want, fmt)
        t.free()
    ctx.close()


def test_float_fold_records():
    """fold_records<float4, true> on the pool image at F_FLOAT: every record is image_ref.record of the
    reference fold over the displayed words -- the alpha byte's change from the loaded value to 1.0 counted
    -- and the accumulator is the one without the option."""
    case, acc, trace = float_inputs()
    ctx = traced(case, RGBA32F, options={_lib.OPT_FOLD_RECORDS: 1})
    ctx.load_accumulator(acc)
    check_pool(ctx, acc, trace)
    alpha_changes = int((image_ref.displayed(acc)[..., 3] != 255).sum())
    assert alpha_changes > 0
    want_recs = []
    for frame in F_FLOAT:
        want = image_ref.fold_rgba32f(frame, acc, trace)
        want_recs.append((frame,) + image_ref.record(acc, want))
        assert want_recs[-1][1] >= alpha_changes
        ctx.load_accumulator(acc)
        ctx.accumulate(frame)
        assert_same_floats(ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA32F), want, f"frame {frame}")
    recs = rec_tuples(ctx.fold_records())
    ctx.close()
    assert recs == want_recs
