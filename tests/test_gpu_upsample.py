"""Guided upsampling on the device (hrt_upsample / hrt_upsample_present / hrt_order_after):
every byte of both footprints, both formats and the present form against the numpy restatement of S19
(tests/upsample_ref.py), NaN compared as NaN.  Sources are a loaded accumulator of adversarial content or a traced
frame; guides are synthetic (one block table sampled at both resolutions) or the real first hits of a low and a high
context of one scene and camera.  Then a filter first, hrt_order_after, what the call leaves alone, the rejections,
and the Python and C++ mirrors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import present_ref
import upsample_ref as U
import variance_ref as V
from helpers import E, SceneCase, _lib
from test_gpu_denoise import FILL, DevBuf, equal, report, synthetic_source

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = np.finfo(F32).max
TRACE, ACCUM = _lib.IMG_TRACE, _lib.IMG_ACCUM
RGBA8, RGBA32F = _lib.FMT_RGBA8, _lib.FMT_RGBA32F
MODES = [_lib.MODE_RGBA8, _lib.MODE_RGBA32F]
# (ws, hs, wt, ht): low -> target
SIZES = [(1, 1, 1, 1), (1, 1, 3, 2), (5, 3, 10, 6), (5, 3, 13, 7), (37, 23, 74, 46), (37, 23, 100, 50), (64, 36, 128, 72),
         (16, 16, 8, 8), (130, 70, 260, 140)]


def native(mode):
    return RGBA8 if mode == _lib.MODE_RGBA8 else RGBA32F


# ---- inputs --------------------------------------------------------------------------------------------------------

def synthetic_guides(ws, hs, wt, ht, seed=2):
    """(low, high) hit records of one synthetic view: a block table of surfaces (misses, sphere and triangle keys, a
    depth and a normal each) sampled at both resolutions by pixel centre, with per-pixel noise in depth and normal,
    some normals off the unit sphere, equal depths, FLT_MAX, one NaN normal per guide, and in the high guide one pixel
    of a surface the low guide does not show (its store takes the fallback)."""
    rng = np.random.default_rng([seed, ws, hs, wt, ht])
    by, bx = max(1, (hs + 5) // 9), max(1, (ws + 6) // 11)
    kind = rng.permutation(by * bx).reshape(by, bx) % 3
    depth = np.round(rng.uniform(2, 9, (by, bx)) * 2) / 2
    normal = rng.normal(size=(by, bx, 3))
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    out = []
    for w, h in ((ws, hs), (wt, ht)):
        y, x = np.mgrid[0:h, 0:w]
        j, i = ((y + 0.5) * by / h).astype(int), ((x + 0.5) * bx / w).astype(int)
        block = j * bx + i
        hits = np.zeros((h, w), dtype=_lib.HIT_DTYPE)
        hits["kind"] = kind[j, i]
        hits["index"] = np.where(hits["kind"] == 0, 0xFFFFFFFF, block + 3)
        hits["mesh"] = np.where(hits["kind"] == 2, block // 2, 0xFFFFFFFF)
        n = normal[j, i] + rng.normal(size=(h, w, 3)) * 0.04
        n = np.where((rng.uniform(size=(h, w)) < 0.1)[..., None], n * rng.uniform(0.5, 2, (h, w, 1)), n)
        hits["normal"] = n
        t = depth[j, i] + np.round(rng.normal(size=(h, w)) * 2) / 8  # many equal depths
        t[rng.uniform(size=(h, w)) < 0.03] = FLT_MAX
        hits["t"] = np.where(hits["kind"] == 0, FLT_MAX, t)
        if w * h >= 15:
            hits["normal"][h // 2, w // 2] = (np.nan, 0.0, 1.0)
        out.append(hits)
    if wt * ht >= 15:
        out[1]["kind"][ht // 3, wt // 3], out[1]["index"][ht // 3, wt // 3] = 1, 0x7FFFFF00
    return out


# (pitch padding, offset, byte order) per present call: a padded pitch in both byte orders
PRESENT_SHOTS = [(20, 16, _lib.PRESENT_B8G8R8A8), (4, 0, _lib.PRESENT_R8G8B8A8)]


def check_all_forms(ctx, low, lo, hi, d_lo, d_hi, footprint, bufs, image=ACCUM, sigmas=U.DEFAULT_SIGMAS, denoise=None,
                    variance=None, what=None):
    """One configuration through both formats (host and device destination) and the present form in both byte orders
    with padded pitches; low is the image the restatement upsamples.  Returns (kept, fallback) of the restatement."""
    ht, wt = hi.shape
    want32, kept, fallback = U.upsample(low, lo, hi, footprint, sigmas, with_info=True)
    want8 = U.upsample(low, lo, hi, footprint, sigmas, fmt_rgba8=True)
    fields = dict(image_id=image, footprint=footprint, sigma_normal=sigmas[0], sigma_depth=sigmas[1])
    dev32, dev8, target = bufs
    for fmt, want, dev in ((RGBA32F, want32, dev32), (RGBA8, want8, dev8)):
        got = ctx.upsample(wt, ht, d_lo.ptr, d_hi.ptr, fmt, denoise, variance, **fields)
        assert equal(got, want), (what, footprint, fmt, "host", report(got, want))
        dev.fill()
        ctx.upsample_into(dev.ptr, want.nbytes, wt, ht, d_lo.ptr, d_hi.ptr, fmt, denoise, variance, **fields)
        raw = dev.read()
        got = raw[:want.nbytes].view(want.dtype).reshape(want.shape)
        assert equal(got, want), (what, footprint, fmt, "device", report(got, want))
        assert (raw[want.nbytes:] == FILL).all(), (what, footprint, fmt)
    for pad, offset, order in PRESENT_SHOTS:
        pitch = wt * 4 + pad
        target.fill()
        t = ctx.upsample_present(target.ptr + offset, ht * pitch, wt, ht, d_lo.ptr, d_hi.ptr, pitch, order, denoise,
                                 variance, **fields)
        ctx.present_wait(t)
        want = present_ref.present_bytes(want8, wt, ht, pitch, order, target.nbytes, offset, FILL)
        assert target.read().tobytes() == want.tobytes(), (what, footprint, "present", order)
    return kept, fallback


def buffers(wt, ht):
    return DevBuf(wt * ht * 16 + 64), DevBuf(wt * ht * 4 + 64), DevBuf(16 + ht * (wt * 4 + 20) + 256)


# ---- 1. synthetic sources and guides at every size ----------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_synthetic_sources_and_guides(size, mode):
    ws, hs, wt, ht = size
    ctx = E.HrtContext((ws, hs), device=0, mode=mode, debug=True)
    src = synthetic_source(ws, hs, mode)
    ctx.load_accumulator(src)
    lo, hi = synthetic_guides(ws, hs, wt, ht)
    d_lo, d_hi = DevBuf(ws * hs * 32).write(lo), DevBuf(wt * ht * 32).write(hi)
    bufs = buffers(wt, ht)
    for footprint in (2, 4):
        kept, fallback = check_all_forms(ctx, src, lo, hi, d_lo, d_hi, footprint, bufs, what=size)
        if ws * hs >= 15:
            # without these a broken weight path could hide behind the fallback
            assert fallback.any() and fallback.mean() < 0.5, (size, footprint, fallback.mean())
        if min(ws, hs) >= footprint and ws * hs >= 15:  # (a 5 x 3 image holds no 4 x 4 footprint)
            assert (kept == footprint * footprint).any(), (size, footprint)
    # other sigmas
    check_all_forms(ctx, src, lo, hi, d_lo, d_hi, 4, bufs, sigmas=(1.5, 0.02), what=size)
    assert ctx.read(ACCUM, native(mode)).tobytes() == src.tobytes()
    assert d_lo.read().tobytes() == lo.tobytes() and d_hi.read().tobytes() == hi.tobytes()
    buffers_guarded, corrupted = ctx.check_guards()
    assert buffers_guarded > 0 and corrupted == 0
    ctx.close()
    for b in (d_lo, d_hi) + bufs:
        b.free()


# ---- 2. traced frames, real first hits of two contexts, hrt_order_after ---------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,size", [("box", (37, 23, 74, 46)), ("box", (16, 16, 8, 8)), ("spheres", (37, 23, 100, 50)),
                                       ("spheres", (64, 36, 128, 72))])
def test_traced_frames_with_real_first_hits(name, size, mode):
    ws, hs, wt, ht = size
    low_case = SceneCase(name, (ws, hs), num_samples=1, max_bounces=2)
    high_case = SceneCase(name, (wt, ht), num_samples=1, max_bounces=2)
    low, high = low_case.context(mode=mode, debug=True), high_case.context(mode=mode)
    for frame in range(2):
        low.trace(low_case.push(1 + frame))
        low.accumulate(frame)
    low.trace(low_case.push(7))  # (the trace image differs from the accumulator)
    d_lo, d_hi = DevBuf(ws * hs * 32), DevBuf(wt * ht * 32)
    low.first_hits(low_case.push(), d_lo.ptr)
    low.synchronize()
    lo = d_lo.read().view(_lib.HIT_DTYPE).reshape(hs, ws)
    # the high guide straight from the second context's stream: no host synchronisation before the upsample
    pitch = wt * 4 + 12
    target = DevBuf(ht * pitch + 64)
    high.first_hits(high_case.push(), d_hi.ptr)
    low.order_after(high)
    ticket = low.upsample_present(target.ptr, ht * pitch, wt, ht, d_lo.ptr, d_hi.ptr, pitch, _lib.PRESENT_B8G8R8A8)
    low.present_wait(ticket)
    hi = d_hi.read().view(_lib.HIT_DTYPE).reshape(ht, wt)
    assert hi.tobytes() == high.intersect_primary(high_case.push()).tobytes()
    assert len(np.unique(D.surface_keys(hi))) >= 3
    srcs = {img: low.read(img, native(mode)) for img in (TRACE, ACCUM)}
    want8 = U.upsample(srcs[ACCUM], lo, hi, fmt_rgba8=True)
    want = present_ref.present_bytes(want8, wt, ht, pitch, present_ref.B8G8R8A8, target.nbytes, 0, FILL)
    assert target.read().tobytes() == want.tobytes()
    bufs = buffers(wt, ht)
    for image in (TRACE, ACCUM):
        for footprint in (2, 4):
            kept, fallback = check_all_forms(low, srcs[image], lo, hi, d_lo, d_hi, footprint, bufs, image=image,
                                             what=(name, size))
            assert fallback.mean() < 0.5 and (kept > 0).any()
    for img in (TRACE, ACCUM):
        assert low.read(img, native(mode)).tobytes() == srcs[img].tobytes(), img
    assert low.check_guards()[1] == 0
    low.close()
    high.close()
    for b in (d_lo, d_hi, target) + bufs:
        b.free()


# ---- 3. a filter first -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_filters_first(mode):
    ws, hs, wt, ht = 37, 23, 74, 46
    ctx = E.HrtContext((ws, hs), device=0, mode=mode, debug=True)
    src = synthetic_source(ws, hs, mode)
    lo, hi = synthetic_guides(ws, hs, wt, ht)
    d_lo, d_hi = DevBuf(ws * hs * 32).write(lo), DevBuf(wt * ht * 32).write(hi)
    ctx.fill_history(6)
    ctx.fill_moments(0.3, 0.2)
    ctx.load_accumulator(src)
    cnt, mom = ctx.read_history(), ctx.read_moments()
    bufs = buffers(wt, ht)
    dn = ctx.denoise_info(iterations=3, sigma_colour=2.0)
    filtered = D.denoise(src, 3, (2.0,) + D.DEFAULT_SIGMAS[1:], lo)
    vi = ctx.variance_info(iterations=2)
    vfiltered, _ = V.denoise_variance(src, cnt, mom, 2, V.DEFAULTS, lo)
    for footprint in (2, 4):
        check_all_forms(ctx, filtered, lo, hi, d_lo, d_hi, footprint, bufs, denoise=dn, what="denoise")
        check_all_forms(ctx, vfiltered, lo, hi, d_lo, d_hi, footprint, bufs, variance=vi, what="variance")
    # the filters' own rejections apply, and a filter of another image is refused
    with pytest.raises(_lib.HrtError, match="iterations"):
        ctx.upsample(wt, ht, d_lo.ptr, d_hi.ptr, RGBA8, ctx.denoise_info(iterations=6))
    with pytest.raises(_lib.HrtError, match="min_history"):
        ctx.upsample(wt, ht, d_lo.ptr, d_hi.ptr, RGBA8, None, ctx.variance_info(min_history=0))
    with pytest.raises(_lib.HrtError, match="image_id"):
        ctx.upsample(wt, ht, d_lo.ptr, d_hi.ptr, RGBA8, ctx.denoise_info(image_id=TRACE))
    with pytest.raises(_lib.HrtError, match="HRT_IMG_ACCUM"):
        ctx.upsample(wt, ht, d_lo.ptr, d_hi.ptr, RGBA8, None, vi, image_id=TRACE)
    assert ctx.read(ACCUM, native(mode)).tobytes() == src.tobytes()
    assert ctx.read_history().tobytes() == cnt.tobytes() and ctx.read_moments().tobytes() == mom.tobytes()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    for b in (d_lo, d_hi) + bufs:
        b.free()


# ---- 4. the call leaves the rest alone -------------------------------------------------------------------------------

def _stats_tuple(st):
    # (timings and wave_steps depend on scheduling: tests/test_gpu_intersect.py)
    return (st.segments, st.tri_tests, st.traces, st.accumulates, st.last_kernel, st.last_block, st.last_frames)


@pytest.mark.parametrize("mode", MODES)
def test_the_call_leaves_the_rest_alone(mode):
    size = ws, hs = 37, 23
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context(mode=mode, debug=True, options={_lib.OPT_FOLD_RECORDS: 1})
    twin = case.context(mode=mode, options={_lib.OPT_FOLD_RECORDS: 1})
    d_lo = DevBuf(ws * hs * 32)
    ctx.intersect_primary_into(case.push(), d_lo.ptr)
    lo = d_lo.read().view(_lib.HIT_DTYPE).reshape(hs, ws)
    plain = DevBuf(ws * hs * 4)

    def old_calls(c, base):
        """hrt_trace, hrt_accumulate, hrt_denoise and hrt_present: the bytes each gives."""
        out = []
        for frame in range(2):
            c.trace(case.push(base + frame))
            c.accumulate(base - 1 + frame)
        out.append(c.read(TRACE, native(mode)))
        out.append(c.read(ACCUM, native(mode)))
        out.append(c.denoise(RGBA32F, d_lo.ptr))
        plain.fill()
        c.present_wait(c.present(ACCUM, plain.ptr, plain.nbytes, ws, hs))
        out.append(plain.read())
        return [a.tobytes() for a in out]

    ctx.fill_history(3)
    ctx.fill_moments(0.5, 0.75)
    assert old_calls(ctx, 1) == old_calls(twin, 1)
    before = {img: ctx.read(img, native(mode)) for img in (TRACE, ACCUM)}
    state = (_stats_tuple(ctx.stats()), ctx.fold_records(with_total=True), ctx.read_history(), ctx.read_moments())
    # targets of different sizes, growing and shrinking: the scratch is reused, the staging image grows once
    for wt, ht in ((20, 9), (100, 50), (74, 46), (100, 50)):
        hi_case = SceneCase("box", (wt, ht), num_samples=1, max_bounces=2)
        high = hi_case.context(mode=mode)
        d_hi = DevBuf(wt * ht * 32)
        high.intersect_primary_into(hi_case.push(), d_hi.ptr)
        hi = d_hi.read().view(_lib.HIT_DTYPE).reshape(ht, wt)
        bufs = buffers(wt, ht)
        for image in (TRACE, ACCUM):
            check_all_forms(ctx, before[image], lo, hi, d_lo, d_hi, 2, bufs, image=image, what=(wt, ht))
        a = ctx.upsample(wt, ht, d_lo.ptr, d_hi.ptr, RGBA32F, footprint=4)
        n = ctx.check_guards()
        assert n[0] > 0 and n[1] == 0
        b = ctx.upsample(wt, ht, d_lo.ptr, d_hi.ptr, RGBA32F, footprint=4)
        assert a.tobytes() == b.tobytes() and ctx.check_guards() == n
        high.close()
        for buf in (d_hi,) + bufs:
            buf.free()
    # nothing else changed: both images, the statistics, the fold records, N and M, the guide
    for img in (TRACE, ACCUM):
        assert ctx.read(img, native(mode)).tobytes() == before[img].tobytes(), img
    assert _stats_tuple(ctx.stats()) == state[0]
    after = ctx.fold_records(with_total=True)
    assert after[1] == state[1][1] and after[0].tobytes() == state[1][0].tobytes()
    assert ctx.read_history().tobytes() == state[2].tobytes() and ctx.read_moments().tobytes() == state[3].tobytes()
    assert d_lo.read().tobytes() == lo.tobytes()
    # ... and the old entry points go on as on a context that never upsampled
    assert old_calls(ctx, 5) == old_calls(twin, 5)
    ctx.close()
    twin.close()
    d_lo.free()
    plain.free()


# ---- 5. the rejections -----------------------------------------------------------------------------------------------

def test_rejections_enqueue_nothing_and_leave_the_context_usable():
    ws, hs, wt, ht = 37, 23, 74, 46
    case = SceneCase("box", (ws, hs), num_samples=1, max_bounces=2)
    ctx = case.context()
    ctx.trace(case.push(1))
    ctx.accumulate(0)
    lib, handle = ctx.lib, ctx.handle
    lo, hi = synthetic_guides(ws, hs, wt, ht)
    d_lo, d_hi = DevBuf(ws * hs * 32 + 16).write(lo), DevBuf(wt * ht * 32 + 16).write(hi)
    host = np.full(wt * ht * 16, FILL, np.uint8)
    target = DevBuf(wt * ht * 4)
    good = ctx.upsample_info(wt, ht)
    before = ctx.upsample(wt, ht, d_lo.ptr, d_hi.ptr, RGBA32F)
    plain = DevBuf(ws * hs * 4)
    t0 = ctx.present(ACCUM, plain.ptr, plain.nbytes, ws, hs)
    ctx.present_wait(t0)
    dn, vi = ctx.denoise_info(), ctx.variance_info()

    def ref(p):
        return ctypes.byref(p) if p is not None else None

    def raw(info=good, denoise=None, variance=None, low=d_lo.ptr, high=d_hi.ptr, fmt=RGBA32F, dst=host.ctypes.data,
            nbytes=host.nbytes):
        return lib.hrt_upsample(handle, ref(info), ref(denoise), ref(variance), ctypes.c_void_p(low or 0),
                                ctypes.c_void_p(high or 0), fmt, ctypes.c_void_p(dst or 0), nbytes)

    def raw_present(info=good, denoise=None, variance=None, low=d_lo.ptr, high=d_hi.ptr, image=ACCUM, dst=target.ptr,
                    nbytes=target.nbytes, size=(wt, ht)):
        pi, t = _lib.PresentInfo(image, _lib.PRESENT_B8G8R8A8, size[0], size[1], size[0] * 4, 0), ctypes.c_uint64(99)
        st = lib.hrt_upsample_present(handle, ref(info), ref(denoise), ref(variance), ctypes.c_void_p(low or 0),
                                      ctypes.c_void_p(high or 0), ctypes.byref(pi), ctypes.c_void_p(dst or 0), nbytes,
                                      ctypes.byref(t))
        assert t.value == 99  # no ticket was issued
        return st

    def altered(**kw):
        info = ctx.upsample_info(wt, ht)
        for k, v in kw.items():
            setattr(info, k, v)
        return info

    bad_infos = [("footprint", 0), ("footprint", 1), ("footprint", 3), ("footprint", 8), ("flags", 1), ("image_id", 2),
                 ("image_id", ACCUM | _lib.IMG_LOCAL), ("width", 0), ("height", 0), ("width", 16385), ("height", 16385)]
    bad_infos += [(s, v) for s in ("sigma_normal", "sigma_depth") for v in (0.0, -1.0, float("nan"), float("inf"))]
    hits_host = np.zeros(wt * ht, dtype=_lib.HIT_DTYPE)
    for call in (raw, raw_present):
        assert call(info=None) == 1 and b"null info" in lib.hrt_last_error(handle)
        for field, value in bad_infos:
            assert call(info=altered(**{field: value})) == 1, (field, value)
            assert b"hrt_upsample" in lib.hrt_last_error(handle)
        assert call(info=altered(footprint=3)) == 1 and b"footprint" in lib.hrt_last_error(handle)
        assert call(info=altered(flags=2)) == 1 and b"flags" in lib.hrt_last_error(handle)
        assert call(info=altered(sigma_depth=0.0)) == 1 and b"sigma" in lib.hrt_last_error(handle)
        assert call(info=altered(width=16385)) == 1 and b"16384" in lib.hrt_last_error(handle)
        assert call(denoise=dn, variance=vi) == 1 and b"at most one" in lib.hrt_last_error(handle)
        assert call(low=None) == 1 and b"null" in lib.hrt_last_error(handle)
        assert call(high=None) == 1 and b"null" in lib.hrt_last_error(handle)
        assert call(low=hits_host.ctypes.data) == 1 and b"low_hits" in lib.hrt_last_error(handle)    # host memory
        assert call(high=hits_host.ctypes.data) == 1 and b"high_hits" in lib.hrt_last_error(handle)
        assert call(low=d_lo.ptr + 8) == 1 and b"aligned" in lib.hrt_last_error(handle)                # misaligned
        assert call(high=d_hi.ptr + 8) == 1 and b"aligned" in lib.hrt_last_error(handle)
        assert call(dst=None) == 1
    assert raw(fmt=7) == 1 and b"format" in lib.hrt_last_error(handle)
    assert raw(nbytes=wt * ht * 16 - 1) == 1 and b"too small" in lib.hrt_last_error(handle)
    assert raw_present(nbytes=target.nbytes - 1) == 1
    assert raw_present(image=TRACE) == 1 and b"image_id" in lib.hrt_last_error(handle)   # differs from info's
    assert raw_present(size=(wt, ht - 1)) == 1 and b"size" in lib.hrt_last_error(handle)  # differs from info's
    assert raw_present(dst=host.ctypes.data, nbytes=wt * ht * 4) == 1                     # pageable host target
    assert (host == FILL).all() and (target.read() == FILL).all()
    # nothing was enqueued or issued: the next ticket follows t0, and the context works as before
    assert ctx.present(ACCUM, plain.ptr, plain.nbytes, ws, hs) == t0 + 1
    assert ctx.upsample(wt, ht, d_lo.ptr, d_hi.ptr, RGBA32F).tobytes() == before.tobytes()
    # hrt_order_after: itself is a no-op, a NULL producer is refused
    ctx.order_after(ctx)
    assert lib.hrt_order_after(handle, None) == 1 and b"producer" in lib.hrt_last_error(handle)
    ctx.close()
    # a row-tile partition, with and without a communicator, and an unpartitioned context joined to one
    parts = [case.context(partition=(8, p, 2)) for p in range(2)]
    for joined in (False, True):
        if joined:
            E.HrtContext.comm_init_all(parts)
        for c in parts:
            with pytest.raises(_lib.HrtError, match="partition"):
                c.upsample(wt, ht, d_lo.ptr, d_hi.ptr)
            with pytest.raises(_lib.HrtError, match="partition"):
                c.upsample_present(target.ptr, target.nbytes, wt, ht, d_lo.ptr, d_hi.ptr)
    for c in parts:
        c.close()
    single = case.context()
    E.HrtContext.comm_init_all([single])
    with pytest.raises(_lib.HrtError, match="communicator"):
        single.upsample(wt, ht, d_lo.ptr, d_hi.ptr)
    single.close()
    for b in (d_lo, d_hi, target, plain):
        b.free()


def test_order_after_rejects_another_device():
    n = ctypes.c_int(0)
    lib = ctypes.CDLL("libamdhip64.so")
    assert lib.hipGetDeviceCount(ctypes.byref(n)) == 0
    if n.value < 2:
        pytest.skip("one device: a pair on different devices cannot be made")
    a, b = E.HrtContext((8, 8), device=0), E.HrtContext((8, 8), device=1)
    with pytest.raises(_lib.HrtError, match="different devices"):
        a.order_after(b)
    a.close()
    b.close()


# ---- 6. the mirrors --------------------------------------------------------------------------------------------------

def test_pipeline_mirror():
    """RenderPassOverFrame.render_upsampled with the high guide from a second pipeline's first_hits_async."""
    (ws, hs), (wt, ht) = (24, 16), (48, 32)
    cam, settings = E.preset("box")
    settings.num_samples, settings.max_bounces = 1, 2
    low, high = E.HrtContext((ws, hs), device=0, mode=_lib.MODE_RGBA32F), E.HrtContext((wt, ht), device=0)
    pipe, diffuse = E.RayTracePipeline(low, (ws, hs), settings), E.DiffusePipeline(low, (ws, hs))
    guide_pipe = E.RayTracePipeline(high, (wt, ht), settings)
    for frame in range(2):
        pipe.compute(cam, frame)
        diffuse.next_frame(frame, pipe.image())
    d_lo, d_hi, target = DevBuf(ws * hs * 32), DevBuf(wt * ht * 32), DevBuf(wt * ht * 4)
    pipe.first_hits_into(cam, d_lo.ptr)
    guide_pipe.first_hits_async(cam, d_hi.ptr)
    rp = E.RenderPassOverFrame(low, _lib.PRESENT_R8G8B8A8)
    pt = E.PresentTarget(target.ptr, target.nbytes, wt, ht, None, _lib.PRESENT_R8G8B8A8)
    low.present_wait(rp.render_upsampled(diffuse.image(), pt, d_lo.ptr, d_hi.ptr, producer=high, footprint=4))
    lo = d_lo.read().view(_lib.HIT_DTYPE).reshape(hs, ws)
    hi = d_hi.read().view(_lib.HIT_DTYPE).reshape(ht, wt)
    assert hi.tobytes() == guide_pipe.first_hits(cam).tobytes()
    want8 = U.upsample(low.read(ACCUM, RGBA32F), lo, hi, 4, fmt_rgba8=True)
    want = present_ref.present_bytes(want8, wt, ht, wt * 4, present_ref.R8G8B8A8, target.nbytes, 0, FILL)
    assert target.read().tobytes() == want.tobytes()
    low.close()
    high.close()
    for b in (d_lo, d_hi, target):
        b.free()


def test_cpp_mirror_upsample(tmp_path):
    """include/hrt_app.hpp's upsample / render_upsampled / order_after (tests/cpp/upsample_demo) give the
    restatement's bytes on the box scene's geometry."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "upsample_demo.mk", "upsample_demo"], check=True)  # (up to date after build())
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
    r = subprocess.run([os.path.join(cpp, "upsample_demo"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    (ws, hs), (w, h) = (24, 16), (48, 32)
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [w, h] and len(raw) == 8 + w * h * (16 + 4)
    up = np.frombuffer(raw[8:8 + w * h * 16], F32).reshape(h, w, 4)
    shown = np.frombuffer(raw[8 + w * h * 16:], np.uint8)
    # the demo's scene through the Python mirror: the same geometry, Lambertian grey, 1 sample, 4 bounces, light on
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    st = E.RayTracerSettings(num_samples=1, max_bounces=4, use_environment_lighting=True,
                             sphere_data=[E.Sphere(s.centre, s.radius, grey) for s in settings.sphere_data],
                             mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in settings.mesh_data])
    low, high = E.HrtContext((ws, hs), device=0, mode=_lib.MODE_RGBA32F), E.HrtContext((w, h), device=0)
    pipe, diffuse, cam = E.RayTracePipeline(low, (ws, hs), st), E.DiffusePipeline(low, (ws, hs)), E.Camera()
    for frame in range(3):
        pipe.compute(cam, frame)
        diffuse.next_frame(frame, pipe.image())
    acc, lo, hi = low.read(ACCUM, RGBA32F), pipe.first_hits(cam), E.RayTracePipeline(high, (w, h), st).first_hits(cam)
    low.close()
    high.close()
    assert equal(up, U.upsample(acc, lo, hi, 4))
    want = present_ref.present_pixels(U.upsample(acc, lo, hi, fmt_rgba8=True), w, h, present_ref.B8G8R8A8)
    assert shown.tobytes() == want.tobytes()
