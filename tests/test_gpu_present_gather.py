"""The gathered present: hrt_present / hrt_accumulate_present on the root of an hrt_comm_init_all group
(interleaved row tiles, one context per part; here all parts share device 0, so the transport is
HRT_COMM_DEVICE_COPY, and a group of one context is HRT_COMM_RCCL_GROUP).  Every expected target is built
in numpy (tests/present_ref.py) from read_frame of the same group or of a twin group that never presents
-- never from another present.  Targets follow tests/test_gpu_present.py: device memory pre-filled with
0xA5, 256 bytes larger than the call is told, the whole allocation compared."""
import ctypes

import numpy as np
import pytest

import present_ref
from epq_raytracer_amd import HrtContext, _lib
from helpers import SceneCase
from test_gpu_present import BGRA, FILL, MODES, RGBA, Target

pytestmark = pytest.mark.gpu

ACCUM, TRACE = _lib.IMG_ACCUM, _lib.IMG_TRACE


def make_group(case, parts, tile, mode=_lib.MODE_RGBA8, debug=False, options=None):
    """parts contexts of tile-row tiles on device 0, joined (part i = ctxs[i]; ctxs[0] is the root)."""
    ctxs = [case.context(mode=mode, partition=(tile, p, parts), debug=debug, options=options) for p in range(parts)]
    HrtContext.comm_init_all(ctxs)
    assert ctxs[0].comm_info() == (0, parts, _lib.COMM_DEVICE_COPY)
    return ctxs


def step(ctxs, case, frame):
    """Frame `frame` on every part: trace, accumulate."""
    for c in ctxs:
        c.trace(case.push(init=True) if frame == 0 else case.push(frame))
        c.accumulate(frame)


def load_random_accumulators(ctxs, seed):
    """Seeded random texels in every part's accumulator, padded local rows included (they must never
    show): every byte lane differs, and RGBA32F values run past both ends of the clamp."""
    rng = np.random.default_rng(seed)
    for c in ctxs:
        shape = (c.local_rows, c.width, 4)
        if c.mode == _lib.MODE_RGBA8:
            c.load_accumulator(rng.integers(0, 256, shape, dtype=np.uint8))
        else:
            c.load_accumulator(rng.uniform(-0.1, 1.1, shape).astype(np.float32))


def rank_major(ctxs, image, height):
    """The frame a wrong row map would show: the parts' blocks in rank order, not un-interleaved."""
    return np.concatenate([c.read(image) for c in ctxs])[:height]


def close_all(ctxs):
    for c in ctxs:
        c.close()


def traced_group(case, parts, tile, mode, seed):
    """A group whose trace image holds frame 2 and whose accumulators hold random texels, with both
    gathered frames read back."""
    ctxs = make_group(case, parts, tile, mode)
    for f in range(2):
        step(ctxs, case, f)
    for c in ctxs:
        c.trace(case.push(2))
    load_random_accumulators(ctxs, seed)
    src = {i: ctxs[0].read_frame(i) for i in (ACCUM, TRACE)}
    return ctxs, src


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene, size, parts, tile", [
    ("island", (80, 70), 2, 8), ("island", (80, 70), 3, 16), ("island", (80, 70), 8, 8), ("island", (80, 70), 5, 4),
    ("box", (37, 23), 3, 4),   # odd width (the 16-byte body row by row), partial last tile
    ("box", (1, 130), 5, 8)])
def test_same_size(scene, size, parts, tile, mode):
    """The root's target holds the full frame flipped and swizzled: both formats, both images, tight and
    padded pitch.  The trace image's target also equals the unpartitioned context's present, byte for byte."""
    w, h = size
    case = SceneCase(scene, size, 2, 8)
    ctxs, src = traced_group(case, parts, tile, mode, seed=parts * 100 + tile)
    root = ctxs[0]
    full = case.context(mode=mode)
    full.trace(case.push(2))
    # precondition: a present that forgot to un-interleave the rows would not pass
    naive = rank_major(ctxs, ACCUM, h)
    assert (naive != src[ACCUM]).any()
    if w * h >= 500:
        assert (rank_major(ctxs, TRACE, h) != src[TRACE]).any() and src[TRACE][..., :3].any()
    assert np.array_equal(src[TRACE], full.read(TRACE))
    for pitch in (w * 4, w * 4 + 12):
        for fmt in (BGRA, RGBA):
            for image in (ACCUM, TRACE):
                t = Target(w, h, pitch)
                ticket = root.present(image, *t.args(), fmt=fmt)
                root.present_wait(ticket)
                assert root.present_done(ticket)
                t.expect(src[image], fmt)
                if image == ACCUM:
                    want, wrong = (present_ref.present_bytes(s, w, h, pitch, fmt, t.buf.nbytes, 0, FILL)
                                   for s in (src[ACCUM], naive))
                    assert (want != wrong).any()
                else:
                    u = Target(w, h, pitch)
                    full.present_wait(full.present(TRACE, *u.args(), fmt=fmt))
                    assert np.array_equal(t.buf.read(), u.buf.read())
                    u.free()
                t.free()
    full.close()
    close_all(ctxs)


@pytest.mark.parametrize("mode", MODES)
def test_scaled(mode):
    """The pinned index rule over the FULL image (Ws = width, Hs = height, not local_rows); 80x70 -> 80x35
    puts every row's sample on a texel edge."""
    size, parts, tile = (80, 70), 3, 16
    case = SceneCase("island", size, 2, 8)
    ctxs, src = traced_group(case, parts, tile, mode, seed=7)
    root = ctxs[0]
    for wt, ht in ((50, 31), (160, 140), (80, 35), (1, 1)):
        for pitch, fmt, image in ((wt * 4, BGRA, ACCUM), (wt * 4 + 12, RGBA, ACCUM), (wt * 4 + 12, BGRA, TRACE)):
            t = Target(wt, ht, pitch)
            root.present_wait(root.present(image, *t.args(), fmt=fmt))
            t.expect(src[image], fmt)
            t.free()
    close_all(ctxs)


@pytest.mark.parametrize("image, defer", [(ACCUM, 0), (ACCUM, 1), (TRACE, 0), (TRACE, 1)])
def test_ordering_and_tickets(image, defer):
    """A gathered present holds every member's image as of the call: frame k's present, then -- with no
    wait -- frame k+1's trace and accumulate on both members and a second present.  The twin group never
    presents; its read-backs after k and k+1 are the references.  Deferred combines are folded by the
    present on every member; with them the trace image is a ring slot (the fold_done record)."""
    size, k = (64, 48), 1
    case = SceneCase("box", size, 2, 4)
    opts = {_lib.OPT_DEFER_COMBINE: defer}
    twin = make_group(case, 2, 8, options=opts)
    step(twin, case, 0)
    step(twin, case, k)
    ref_k = twin[0].read_frame(image)
    step(twin, case, k + 1)
    ref_k1 = twin[0].read_frame(image)
    close_all(twin)
    assert (ref_k != ref_k1).any()

    ctxs = make_group(case, 2, 8, options=opts)
    root = ctxs[0]
    a, b = Target(*size), Target(*size)
    step(ctxs, case, 0)
    step(ctxs, case, k)
    ta = root.present(image, *a.args())
    step(ctxs, case, k + 1)
    tb = root.present(image, *b.args())
    assert (ta, tb) == (1, 2)
    root.synchronize()
    assert root.present_done(ta) and root.present_done(tb)
    a.expect(ref_k, BGRA)
    b.expect(ref_k1, BGRA)
    # the members went on undisturbed: the group's frame is the twin's
    assert np.array_equal(root.read_frame(image), ref_k1)
    close_all(ctxs)
    a.free()
    b.free()


@pytest.mark.parametrize("mode", MODES)
def test_accumulate_present_on_the_root(mode):
    """hrt_accumulate_present on the root against a twin group that calls hrt_accumulate on each member
    and hrt_present on the root: frames 0..2 at the image's size, frame 3 into a scaled target.  Same
    targets, same gathered accumulator, same accumulate count on every member, no guard band touched."""
    size, scaled, parts, tile = (37, 23), (50, 31), 3, 4
    native = _lib.FMT_RGBA8 if mode == _lib.MODE_RGBA8 else _lib.FMT_RGBA32F
    case = SceneCase("box", size, 2, 4)
    fused, twin = make_group(case, parts, tile, mode, debug=True), make_group(case, parts, tile, mode, debug=True)
    shapes = [size] * 3 + [scaled]
    ft = [Target(*s, pitch=s[0] * 4 + 12) for s in shapes]
    tt = [Target(*s, pitch=s[0] * 4 + 12) for s in shapes]
    for f, (a, b) in enumerate(zip(ft, tt)):
        fmt = BGRA if f % 2 == 0 else RGBA
        for c in fused + twin:
            c.trace(case.push(init=True) if f == 0 else case.push(f))
        assert fused[0].accumulate_present(f, *a.args(), fmt=fmt) == f + 1
        for c in twin:
            c.accumulate(f)
        assert twin[0].present(ACCUM, *b.args(), fmt=fmt) == f + 1
        ref = twin[0].read_frame(ACCUM)  # the numpy reference of this frame (a blocking read)
        fused[0].present_wait(f + 1)
        a.expect(ref, fmt)
        b.expect(ref, fmt)
        assert np.array_equal(a.buf.read(), b.buf.read())
    got, want = fused[0].read_frame(ACCUM, native), twin[0].read_frame(ACCUM, native)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)) and fused[0].read_frame(ACCUM)[..., :3].any()
    for c, d in zip(fused, twin):
        assert c.stats().accumulates == d.stats().accumulates == len(shapes)
    for c in fused + twin:
        n, bad = c.check_guards()
        assert n > 0 and bad == 0
    close_all(fused + twin)
    for t in ft + tt:
        t.free()


@pytest.mark.parametrize("mode", MODES)
def test_single_rank_rccl_group(mode):
    """comm_init_all([ctx]) forms an HRT_COMM_RCCL_GROUP of one: the grouped ncclGather feeds the same
    kernel, and the target equals the one the context wrote before it joined."""
    size = (64, 48)
    case = SceneCase("box", size, 2, 4)
    ctx = case.context(mode=mode)
    step([ctx], case, 0)
    step([ctx], case, 1)
    ctx.trace(case.push(2))
    src = {i: ctx.read(i) for i in (ACCUM, TRACE)}
    shots = [(ACCUM, size, BGRA), (TRACE, size, RGBA), (ACCUM, (50, 31), RGBA)]
    before = [Target(*s, pitch=s[0] * 4 + 12) for _, s, _ in shots]
    for (image, _, fmt), t in zip(shots, before):
        ctx.present_wait(ctx.present(image, *t.args(), fmt=fmt))
    HrtContext.comm_init_all([ctx])
    assert ctx.comm_info() == (0, 1, _lib.COMM_RCCL_GROUP)
    for (image, s, fmt), old in zip(shots, before):
        t = Target(*s, pitch=s[0] * 4 + 12)
        ctx.present_wait(ctx.present(image, *t.args(), fmt=fmt))
        t.expect(src[image], fmt)
        assert np.array_equal(t.buf.read(), old.buf.read())
        t.free()
        old.free()
    last = Target(*size)
    assert ctx.accumulate_present(2, *last.args()) == 7  # (three tickets before the group, three in it)
    ctx.present_wait(7)
    last.expect(ctx.read_frame(ACCUM), BGRA)
    assert ctx.stats().accumulates == 3
    last.free()
    ctx.close()


def test_validation():
    """Who may present: only the root of an intact hrt_comm_init_all group.  Every rejection is
    HRT_ERR_INVALID_ARGUMENT decided on the host: the target stays untouched, no ticket is issued, no
    member accumulates."""
    size = (37, 23)
    w, h = size
    case = SceneCase("box", size, 2, 4)
    ctxs = make_group(case, 2, 8)
    root, other = ctxs
    step(ctxs, case, 0)
    lone = case.context()
    step([lone], case, 0)
    lone.comm_init(HrtContext.comm_unique_id(), 0, 1)
    t = Target(w, h, w * 4 + 12)
    need = (h - 1) * t.pitch + w * 4

    def rejected(call, match):
        with pytest.raises(_lib.HrtError, match="INVALID") as e:
            call()
        assert match in str(e.value), str(e.value)

    rejected(lambda: other.present(ACCUM, *t.args()), "root")            # a member other than the root
    rejected(lambda: other.accumulate_present(1, *t.args()), "root")
    rejected(lambda: lone.present(ACCUM, *t.args()), "hrt_comm_init")     # a process communicator
    rejected(lambda: lone.accumulate_present(1, *t.args()), "hrt_comm_init")
    # bad arguments on the root, one of each kind
    rejected(lambda: root.present(2, *t.args()), "image")
    rejected(lambda: root.present(ACCUM | _lib.IMG_LOCAL, *t.args()), "image")
    rejected(lambda: root.accumulate_present(1, *t.args(), fmt=7), "format")
    rejected(lambda: root.present(ACCUM, t.ptr, t.claimed, 0, h, t.pitch), "width")
    rejected(lambda: root.present(ACCUM, t.ptr, t.claimed, w, 16385, t.pitch), "height")
    rejected(lambda: root.present(ACCUM, t.ptr, t.claimed, w, h, w * 4 - 4), "pitch")
    rejected(lambda: root.present(ACCUM, t.ptr, t.claimed, w, h, w * 4 + 2), "pitch")
    rejected(lambda: root.present(ACCUM, t.ptr + 2, t.claimed, w, h, t.pitch), "aligned")
    rejected(lambda: root.present(ACCUM, t.ptr, need - 1, w, h, t.pitch), "smaller")
    rejected(lambda: root.accumulate_present(1, t.ptr, need - 1, w, h, t.pitch), "smaller")
    host = np.full(t.claimed, FILL, np.uint8)                              # pageable host memory
    rejected(lambda: root.present(ACCUM, host.ctypes.data, host.nbytes, w, h, t.pitch), "destination")
    assert (host == FILL).all()
    info = _lib.PresentInfo(ACCUM, BGRA, w, h, t.pitch, 1)                 # flags
    ticket = ctypes.c_uint64(0)
    assert root.lib.hrt_present(root.handle, ctypes.byref(info), ctypes.c_void_p(t.ptr), t.claimed,
                                ctypes.byref(ticket)) == 1
    assert root.lib.hrt_present(root.handle, None, ctypes.c_void_p(t.ptr), t.claimed, ctypes.byref(ticket)) == 1
    assert ticket.value == 0
    for c in (root, other, lone):
        c.synchronize()
        assert c.stats().accumulates == 1
    assert t.untouched()
    for c in (root, other):
        with pytest.raises(_lib.HrtError, match="INVALID"):                # no ticket was issued
            c.present_done(1)
    # a valid present: the minimum size is accepted
    assert root.present(ACCUM, t.ptr, need, w, h, t.pitch) == 1
    root.present_wait(1)
    t.expect(root.read_frame(ACCUM), BGRA)
    # a group with a destroyed member
    u = Target(w, h)
    other.close()
    rejected(lambda: root.present(ACCUM, *u.args()), "destroyed")
    rejected(lambda: root.accumulate_present(1, *u.args()), "destroyed")
    root.synchronize()
    assert u.untouched() and root.stats().accumulates == 1
    with pytest.raises(_lib.HrtError, match="INVALID"):
        root.present_done(2)
    root.close()
    lone.close()
    t.free()
    u.free()


@pytest.mark.parametrize("mode", MODES)
def test_interleaved_with_reads(mode):
    """present, read_frame, present on one group with no wait in between: the gather buffer is reused by
    all three (stream order on the root), so the first target must not show the trace image the read
    gathered right behind it, nor the read the accumulator."""
    size, parts, tile = (37, 23), 3, 4
    case = SceneCase("box", size, 2, 4)
    ctxs, src = traced_group(case, parts, tile, mode, seed=11)
    root = ctxs[0]
    assert (src[ACCUM] != src[TRACE]).any()
    a, b = Target(*size), Target(50, 31, 50 * 4 + 12)
    ta = root.present(ACCUM, *a.args())
    got = root.read_frame(TRACE)
    tb = root.present(ACCUM, *b.args(), fmt=RGBA)
    assert (ta, tb) == (1, 2)
    root.synchronize()
    assert np.array_equal(got, src[TRACE])
    a.expect(src[ACCUM], BGRA)
    b.expect(src[ACCUM], RGBA)
    close_all(ctxs)
    a.free()
    b.free()
