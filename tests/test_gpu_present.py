"""The present pass on the device (hrt_present, hrt_accumulate_present, tickets): every expected target is
built in numpy (tests/present_ref.py: the flip, the pinned index rule, the channel swap) from ctx.read() of
the same context or of a twin that never presents -- never from another present.  Targets are device
memory (hipMalloc through ctypes), pre-filled with 0xA5 and 256 bytes larger than the call is told, so a
write outside the rows (pitch padding, past the end) shows.  Scene box, 2 spp, 4 bounces."""
import ctypes

import numpy as np
import pytest

import present_ref
from epq_raytracer_amd import _lib
from helpers import SceneCase

pytestmark = pytest.mark.gpu

FILL, SLACK = 0xA5, 256
BGRA, RGBA = _lib.PRESENT_B8G8R8A8, _lib.PRESENT_R8G8B8A8
MODES = [_lib.MODE_RGBA8, _lib.MODE_RGBA32F]
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
        self.fill()

    def fill(self):
        assert hip().hipMemset(self.ptr, FILL, self.nbytes) == 0
        assert hip().hipDeviceSynchronize() == 0  # (the contexts' streams do not wait for the null stream)

    def read(self):
        out = np.empty(self.nbytes, np.uint8)
        assert hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0  # device to host
        return out

    def free(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = 0


class Target:
    """A wt x ht present target at `offset` bytes into its own allocation, which is SLACK bytes larger
    than the dst_bytes the call is given."""

    def __init__(self, wt, ht, pitch=None, offset=0):
        self.wt, self.ht, self.pitch, self.offset = wt, ht, wt * 4 if pitch is None else pitch, offset
        self.claimed = self.ht * self.pitch
        self.buf = DevBuf(offset + self.claimed + SLACK)
        self.ptr = self.buf.ptr + offset

    def args(self):
        return self.ptr, self.claimed, self.wt, self.ht, self.pitch

    def expect(self, src, fmt):
        """The allocation's bytes must be what a present of src (hs, ws, 4 uint8) leaves."""
        want = present_ref.present_bytes(src, self.wt, self.ht, self.pitch, fmt, self.buf.nbytes, self.offset, FILL)
        got = self.buf.read()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{bad.size} bytes differ, first at allocation byte {bad[0]} "
                               f"(row {(bad[0] - self.offset) // self.pitch}): {got[bad[0]]} != {want[bad[0]]}")

    def untouched(self):
        return bool((self.buf.read() == FILL).all())

    def free(self):
        self.buf.free()


def traced(size, mode, debug=False, options=None):
    """A context whose accumulator holds frames 0..1 and whose trace image holds frame 2."""
    case = SceneCase("box", size, 2, 4)
    ctx = case.context(mode=mode, debug=debug, options=options)
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    ctx.trace(case.push(1))
    ctx.accumulate(1)
    ctx.trace(case.push(2))
    return case, ctx


@pytest.fixture(scope="module")
def contexts():
    """One traced context per (size, mode), shared by the cases that only present from it, with its two
    images read back once."""
    cache = {}

    def get(size, mode):
        if (size, mode) not in cache:
            _, ctx = traced(size, mode)
            if size[0] * size[1] < 500:
                # the strips and the single pixel see little of the box (300x1 renders black): their
                # accumulator is loaded with random texels, alpha included, so every byte lane shows
                rng = np.random.default_rng(size[0] * 1000 + size[1])
                if mode == _lib.MODE_RGBA8:
                    ctx.load_accumulator(rng.integers(0, 256, (size[1], size[0], 4), dtype=np.uint8))
                else:
                    ctx.load_accumulator(rng.uniform(-0.1, 1.1, (size[1], size[0], 4)).astype(np.float32))
            src = {i: ctx.read(i) for i in (_lib.IMG_ACCUM, _lib.IMG_TRACE)}
            if size[0] * size[1] >= 500:
                assert src[_lib.IMG_ACCUM][..., :3].any() and (src[_lib.IMG_ACCUM] != src[_lib.IMG_TRACE]).any()
            else:
                assert len(np.unique(src[_lib.IMG_ACCUM])) > 1
            cache[(size, mode)] = (ctx, src)
        return cache[(size, mode)]

    yield get
    for ctx, _ in cache.values():
        ctx.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [(37, 23), (64, 48), (1, 1), (300, 1), (1, 130)])
def test_same_size(contexts, size, mode):
    """dst(x, y) = src(x, H-1-y), swizzled: both formats, both images, tight and padded pitch; the odd
    width runs the 16-byte body on the rows that start on a 16-byte boundary, its tail, and the word
    path on the other rows."""
    ctx, src = contexts(size, mode)
    w, h = size
    for pitch in (w * 4, w * 4 + 12):
        for fmt in (BGRA, RGBA):
            for image in (_lib.IMG_ACCUM, _lib.IMG_TRACE):
                t = Target(w, h, pitch)
                ticket = ctx.present(image, *t.args(), fmt=fmt)
                ctx.present_wait(ticket)
                assert ctx.present_done(ticket)
                t.expect(src[image], fmt)
                t.free()


@pytest.mark.parametrize("mode", MODES)
def test_same_size_unaligned_base(contexts, mode):
    """dst 4 bytes past a 16-byte boundary: no row of the target is 16-byte aligned (the word path)."""
    ctx, src = contexts((64, 48), mode)
    for fmt in (BGRA, RGBA):
        t = Target(64, 48, offset=4)
        assert t.ptr % 16 == 4
        ctx.present_wait(ctx.present(_lib.IMG_ACCUM, *t.args(), fmt=fmt))
        t.expect(src[_lib.IMG_ACCUM], fmt)
        t.free()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size, target", [((37, 23), (50, 31)), ((37, 23), (16, 9)), ((37, 23), (74, 46)),
                                          ((37, 23), (1, 1)), ((64, 48), (32, 96)), ((64, 48), (64, 24))])
def test_scaled(contexts, size, target, mode):
    """The pinned index rule; 64x48 -> 32x96 puts every column's sample on a texel edge (Ws = 2 Wt) and
    64x48 -> 64x24 every row's (Hs = 2 Ht)."""
    ctx, src = contexts(size, mode)
    wt, ht = target
    for pitch, fmt, image in ((wt * 4, BGRA, _lib.IMG_ACCUM), (wt * 4 + 12, RGBA, _lib.IMG_ACCUM),
                              (wt * 4 + 12, BGRA, _lib.IMG_TRACE)):
        t = Target(wt, ht, pitch)
        ctx.present_wait(ctx.present(image, *t.args(), fmt=fmt))
        t.expect(src[image], fmt)
        t.free()


def test_ordering_and_tickets():
    """A present holds the image as of the call: frame k's present, then -- with no wait -- frame k+1's
    trace, accumulate and present.  The twin run never presents; its read-backs after k and k+1 are the
    references."""
    size, k = (64, 48), 1
    case = SceneCase("box", size, 2, 4)
    twin = case.context()
    twin.trace(case.push(init=True))
    twin.accumulate(0)
    twin.trace(case.push(k))
    twin.accumulate(k)
    ref_k = twin.read(_lib.IMG_ACCUM)
    twin.trace(case.push(k + 1))
    twin.accumulate(k + 1)
    ref_k1 = twin.read(_lib.IMG_ACCUM)
    twin.close()
    assert (ref_k != ref_k1).any()

    ctx = case.context()
    a, b = Target(*size), Target(*size)
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    ctx.trace(case.push(k))
    ctx.accumulate(k)
    for bad in (0, 99):  # no ticket issued yet / never issued
        with pytest.raises(_lib.HrtError, match="INVALID"):
            ctx.present_done(bad)
        with pytest.raises(_lib.HrtError, match="INVALID"):
            ctx.present_wait(bad)
    ta = ctx.present(_lib.IMG_ACCUM, *a.args())
    ctx.trace(case.push(k + 1))
    ctx.accumulate(k + 1)
    tb = ctx.present(_lib.IMG_ACCUM, *b.args())
    assert (ta, tb) == (1, 2)
    ctx.present_wait(tb)
    ctx.present_wait(ta)
    assert ctx.present_done(ta) and ctx.present_done(tb)
    for bad in (0, 99):
        with pytest.raises(_lib.HrtError, match="INVALID"):
            ctx.present_done(bad)
    a.expect(ref_k, BGRA)
    b.expect(ref_k1, BGRA)
    ctx.close()
    a.free()
    b.free()


def test_ticket_ring():
    """20 presents back to back, no waits, into 8 rotating targets (a call that finds 8 in flight waits for
    the oldest, so a target is rewritten only after its earlier present): every ticket is done after
    synchronize and the last 8 targets hold frames 13..20."""
    size, n = (37, 23), 20
    case = SceneCase("box", size, 2, 4)
    twin = case.context()
    twin.trace(case.push(init=True))
    twin.accumulate(0)
    refs = {}
    for f in range(1, n + 1):
        twin.trace(case.push(f))
        twin.accumulate(f)
        if f > n - _lib.PRESENT_RING:
            refs[f] = twin.read(_lib.IMG_ACCUM)
    twin.close()

    ctx = case.context()
    targets = [Target(*size, pitch=size[0] * 4 + 12) for _ in range(_lib.PRESENT_RING)]
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    tickets = []
    for f in range(1, n + 1):
        ctx.trace(case.push(f))
        ctx.accumulate(f)
        tickets.append(ctx.present(_lib.IMG_ACCUM, *targets[(f - 1) % len(targets)].args(), fmt=RGBA))
    assert tickets == list(range(1, n + 1))
    ctx.synchronize()
    assert all(ctx.present_done(t) for t in tickets)
    for f in range(n - _lib.PRESENT_RING + 1, n + 1):
        targets[(f - 1) % len(targets)].expect(refs[f], RGBA)
    ctx.close()
    for t in targets:
        t.free()


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_accumulate_present(mode, defer):
    """hrt_accumulate_present against a twin that calls hrt_accumulate and hrt_present: frames 0..4 at the
    image's size (one kernel when combines are not deferred) and frame 5 into a scaled target.  Same
    accumulator bytes, same targets, same accumulate count, no guard band touched (debug library)."""
    size, scaled = (37, 23), (50, 31)
    native = _lib.FMT_RGBA8 if mode == _lib.MODE_RGBA8 else _lib.FMT_RGBA32F
    case = SceneCase("box", size, 2, 4)
    opts = {_lib.OPT_DEFER_COMBINE: defer}
    fused, twin = case.context(mode=mode, debug=True, options=opts), case.context(mode=mode, debug=True, options=opts)
    shapes = [size] * 5 + [scaled]
    ft = [Target(*s, pitch=s[0] * 4 + 12) for s in shapes]
    tt = [Target(*s, pitch=s[0] * 4 + 12) for s in shapes]
    for f, (a, b) in enumerate(zip(ft, tt)):
        fmt = BGRA if f % 2 == 0 else RGBA
        for ctx in (fused, twin):
            ctx.trace(case.push(init=True) if f == 0 else case.push(f))
        assert fused.accumulate_present(f, *a.args(), fmt=fmt) == f + 1
        twin.accumulate(f)
        assert twin.present(_lib.IMG_ACCUM, *b.args(), fmt=fmt) == f + 1
        # the numpy reference of this frame, from the twin's accumulator (a blocking read: frame by frame)
        ref = twin.read(_lib.IMG_ACCUM)
        fused.present_wait(f + 1)
        a.expect(ref, fmt)
        b.expect(ref, fmt)
        assert np.array_equal(a.buf.read(), b.buf.read())
    assert np.array_equal(fused.read(_lib.IMG_ACCUM, native), twin.read(_lib.IMG_ACCUM, native))
    assert fused.read(_lib.IMG_ACCUM)[..., :3].any()
    assert fused.stats().accumulates == twin.stats().accumulates == len(shapes)
    for ctx in (fused, twin):
        n, bad = ctx.check_guards()
        assert n > 0 and bad == 0
        ctx.close()
    for t in ft + tt:
        t.free()


def test_present_into_imported_memory():
    """The target is memory the presenting API exported as an fd (here HIP's VMM API) and the context
    imported: accepted by the import's recorded range, read back through the exporter's own mapping."""
    lib = _lib.load()
    size = (64, 48)
    nbytes = size[0] * size[1] * 4
    fd, ptr, mapped = ctypes.c_int32(-1), ctypes.c_void_p(), ctypes.c_uint64()
    st = lib.hrt_debug_export_memory(0, nbytes + SLACK, ctypes.byref(fd), ctypes.byref(ptr), ctypes.byref(mapped))
    if st != 0:
        pytest.skip("device memory export unsupported here: " + lib.hrt_last_error(None).decode())
    _, ctx = traced(size, _lib.MODE_RGBA8)
    assert hip().hipMemset(ptr, FILL, nbytes + SLACK) == 0 and hip().hipDeviceSynchronize() == 0
    dev = ctx.import_external(fd.value, mapped.value, 0, nbytes + SLACK)
    ctx.present_wait(ctx.present(_lib.IMG_ACCUM, dev, nbytes, *size))
    got = np.empty(nbytes + SLACK, np.uint8)
    assert hip().hipMemcpy(got.ctypes.data, ptr, got.nbytes, 2) == 0
    src = ctx.read(_lib.IMG_ACCUM)
    ctx.release_external(dev)
    ctx.close()
    assert lib.hrt_debug_unmap_memory(ptr, mapped.value) == 0
    want = present_ref.present_bytes(src, size[0], size[1], size[0] * 4, BGRA, nbytes + SLACK, 0, FILL)
    np.testing.assert_array_equal(got, want)


def test_validation():
    """Every rejection is HRT_ERR_INVALID_ARGUMENT from the host-side checks, before anything is enqueued:
    the target stays untouched and no ticket is issued."""
    size = (37, 23)
    w, h = size
    _, ctx = traced(size, _lib.MODE_RGBA8)
    lib, handle = ctx.lib, ctx.handle
    t = Target(w, h, w * 4 + 12)
    dst, nbytes, pitch = t.ptr, t.claimed, t.pitch
    ticket = ctypes.c_uint64(0)

    def raw(info, dst=dst, nbytes=nbytes, ticket_ref=ctypes.byref(ticket)):
        return lib.hrt_present(handle, None if info is None else ctypes.byref(info), ctypes.c_void_p(dst), nbytes,
                               ticket_ref)

    def info(image=_lib.IMG_ACCUM, fmt=BGRA, width=w, height=h, pitch=pitch, flags=0):
        return _lib.PresentInfo(image, fmt, width, height, pitch, flags)

    assert raw(None) == 1                                  # null info
    assert raw(info(), dst=0) == 1                         # null destination
    assert raw(info(), ticket_ref=None) == 1               # null ticket
    assert raw(info(image=2)) == 1                         # unknown image ids
    assert raw(info(image=_lib.IMG_ACCUM | _lib.IMG_LOCAL)) == 1
    assert raw(info(fmt=2)) == 1                           # unknown format
    assert raw(info(flags=1)) == 1                         # flags
    for bad in (dict(width=0), dict(height=0), dict(width=16385, pitch=16385 * 4), dict(height=16385)):
        assert raw(info(**bad)) == 1                       # zero / oversized target
    assert raw(info(pitch=w * 4 - 4)) == 1                 # pitch below the row
    assert raw(info(pitch=w * 4 + 2)) == 1                 # pitch not a multiple of 4
    assert raw(info(), dst=dst + 2) == 1                   # misaligned destination
    need = (h - 1) * pitch + w * 4
    assert raw(info(), nbytes=need - 1) == 1               # one byte short
    assert b"hrt_present" in lib.hrt_last_error(handle)
    host = np.full(nbytes, FILL, np.uint8)                 # pageable host memory: refused by the pointer check
    assert raw(info(), dst=host.ctypes.data) == 1
    assert (host == FILL).all()
    # hrt_accumulate_present: the same checks, and only the accumulator
    st = lib.hrt_accumulate_present(handle, 3, ctypes.byref(info(image=_lib.IMG_TRACE)), ctypes.c_void_p(dst), nbytes,
                                    ctypes.byref(ticket))
    assert st == 1
    st = lib.hrt_accumulate_present(handle, 3, ctypes.byref(info()), ctypes.c_void_p(dst), need - 1, ctypes.byref(ticket))
    assert st == 1
    with pytest.raises(_lib.HrtError, match="INVALID"):
        ctx.present(_lib.IMG_ACCUM, *t.args(), fmt=7)
    assert ticket.value == 0 and ctx.stats().accumulates == 2
    with pytest.raises(_lib.HrtError, match="INVALID"):    # no ticket was issued by any of the above
        ctx.present_done(1)
    # a context of a row-tile partition: rejected (the gathered present is a follow-up)
    case = SceneCase("box", size, 2, 4)
    part = case.context(partition=(8, 1, 3))
    with pytest.raises(_lib.HrtError, match="INVALID"):
        part.present(_lib.IMG_ACCUM, *t.args())
    with pytest.raises(_lib.HrtError, match="INVALID"):
        part.accumulate_present(1, *t.args())
    part.close()
    ctx.synchronize()
    assert t.untouched()
    # the minimum size is accepted
    assert raw(info(), nbytes=need) == 0 and ticket.value == 1
    ctx.present_wait(1)
    t.expect(ctx.read(_lib.IMG_ACCUM), BGRA)
    ctx.close()
    t.free()
