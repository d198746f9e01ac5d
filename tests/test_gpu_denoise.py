"""The denoise pass on the device (hrt_denoise / hrt_denoise_present): every byte of
every method against the numpy restatement of S14 (tests/denoise_ref.py), NaN compared as NaN.  Sources are a
traced frame (either image) or a loaded accumulator of adversarial content; guides are NULL, the real first
hits of box and spheres written by hrt_intersect_primary into device memory, and a synthetic guide.  Then the
properties of the call (nothing else changes, guard bands, scratch reuse), hrt_denoise_present against
tests/present_ref.py, the rejections, and the C++ mirror's demo."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import present_ref
from helpers import E, SceneCase, _lib
from image_ref import same_floats

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = np.finfo(F32).max
FILL = 0xA5
TRACE, ACCUM = _lib.IMG_TRACE, _lib.IMG_ACCUM
RGBA8, RGBA32F = _lib.FMT_RGBA8, _lib.FMT_RGBA32F
MODES = [_lib.MODE_RGBA8, _lib.MODE_RGBA32F]
METHODS = [_lib.DENOISE_DIRECT, _lib.DENOISE_TILED, _lib.DENOISE_AUTO]
SIZES = [(1, 1), (5, 3), (37, 23), (64, 36), (130, 70)]  # (width, height)
SIGMAS = D.DEFAULT_SIGMAS
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
    equal values and FLT_MAX; one NaN normal (the comparison rule gives its taps weight 0)."""
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
    hits["normal"] = np.where((rng.uniform(size=(h, w)) < 0.5)[..., None], smooth, unit * rng.uniform(0.5, 2, (h, w, 1)))
    t = np.round(rng.uniform(1, 9, (h, w)) * 4) / 4  # many equal depths
    t[rng.uniform(size=(h, w)) < 0.05] = FLT_MAX
    hits["t"] = np.where(hits["kind"] == 0, FLT_MAX, t)
    if w * h >= 15:
        hits["normal"][h // 2, w // 2] = (np.nan, 0.0, 1.0)
    return hits


def equal(got, want):
    if want.dtype == np.uint8:
        return got.tobytes() == want.tobytes()
    return bool(same_floats(got, want).all())


def report(got, want):
    bad = np.argwhere(~same_floats(got, want).all(-1)) if want.dtype != np.uint8 else np.argwhere((got != want).any(-1))
    y, x = bad[0]
    return f"{len(bad)} pixels differ; first at (x={x}, y={y}): {got[y, x]} vs {want[y, x]}"


def check_call(ctx, want32, want8, guide_ptr, info_fields, dev32, dev8):
    """One configuration through both formats, into host memory and into device memory."""
    for fmt, want, dev in ((RGBA32F, want32, dev32), (RGBA8, want8, dev8)):
        got = ctx.denoise(fmt, guide_ptr, **info_fields)
        assert equal(got, want), (info_fields, fmt, "host", report(got, want))
        dev.fill()
        ctx.denoise_into(dev.ptr, want.nbytes, fmt, guide_ptr, **info_fields)
        raw = dev.read()
        got = raw[:want.nbytes].view(want.dtype).reshape(want.shape)
        assert equal(got, want), (info_fields, fmt, "device", report(got, want))
        assert (raw[want.nbytes:] == FILL).all(), (info_fields, fmt)


# ---- 1. synthetic sources and guides at every size --------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_synthetic_sources_and_guides(size, mode):
    w, h = size
    ctx = E.HrtContext(size, device=0, mode=mode, debug=True)
    src = synthetic_source(w, h, mode)
    ctx.load_accumulator(src)
    hits = synthetic_guide(w, h)
    d_guide = DevBuf(w * h * 32).write(hits)
    dev32, dev8 = DevBuf(w * h * 16 + 64), DevBuf(w * h * 4 + 64)
    for guide, guide_ptr in ((None, None), (hits, d_guide.ptr)):
        for iterations in (1, 3, 5):
            want32 = D.denoise(src, iterations, SIGMAS, guide)
            want8 = D.denoise(src, iterations, SIGMAS, guide, fmt_rgba8=True)
            for method in METHODS:
                check_call(ctx, want32, want8, guide_ptr, dict(image_id=ACCUM, iterations=iterations, method=method),
                           dev32, dev8)
    # other sigmas, and the debug library's two forms of the tiled kernel at every step
    odd = (0.37, 1.5, 0.02)
    want32, want8 = D.denoise(src, 5, odd, hits), D.denoise(src, 5, odd, hits, fmt_rgba8=True)
    for method in METHODS + [_lib.DEBUG_DENOISE_DENSE, _lib.DEBUG_DENOISE_LATTICE]:
        check_call(ctx, want32, want8, d_guide.ptr,
                   dict(image_id=ACCUM, iterations=5, method=method, sigma_colour=odd[0], sigma_normal=odd[1],
                        sigma_depth=odd[2]), dev32, dev8)
    assert ctx.read(ACCUM, RGBA8 if mode == _lib.MODE_RGBA8 else RGBA32F).tobytes() == src.tobytes()
    buffers, corrupted = ctx.check_guards()
    assert buffers > 0 and corrupted == 0
    ctx.close()
    for b in (d_guide, dev32, dev8):
        b.free()


# ---- 2. traced frames, real first hits, and what the call leaves alone ------------------------------------------

def _stats_tuple(st):
    # (timings and wave_steps depend on scheduling: tests/test_gpu_intersect.py)
    return (st.segments, st.tri_tests, st.traces, st.accumulates, st.last_kernel, st.last_block, st.last_frames)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,size", [("box", (64, 36)), ("spheres", (130, 70))])
def test_traced_frames_with_real_first_hits(name, size, mode):
    w, h = size
    native = RGBA8 if mode == _lib.MODE_RGBA8 else RGBA32F
    case = SceneCase(name, size, num_samples=1, max_bounces=4)
    ctx = case.context(mode=mode, debug=True, options={_lib.OPT_FOLD_RECORDS: 1})
    for frame in range(3):
        ctx.trace(case.push(1 + frame))
        ctx.accumulate(frame)
    d_guide = DevBuf(w * h * 32)
    ctx.intersect_primary_into(case.push(), d_guide.ptr)
    hits = d_guide.read().view(_lib.HIT_DTYPE).reshape(h, w)
    assert hits.tobytes() == ctx.intersect_primary(case.push()).tobytes()
    assert len(np.unique(D.surface_keys(hits))) >= 3
    before = {img: ctx.read(img, native) for img in (TRACE, ACCUM)}
    stats, records = _stats_tuple(ctx.stats()), ctx.fold_records(with_total=True)
    dev32, dev8 = DevBuf(w * h * 16 + 64), DevBuf(w * h * 4 + 64)
    for image in (TRACE, ACCUM):
        for guide, guide_ptr in ((hits, d_guide.ptr), (None, None)):
            for iterations in (1, 3, 5) if guide is not None else (5,):
                want32 = D.denoise(before[image], iterations, SIGMAS, guide)
                want8 = D.denoise(before[image], iterations, SIGMAS, guide, fmt_rgba8=True)
                for method in METHODS:
                    check_call(ctx, want32, want8, guide_ptr, dict(image_id=image, iterations=iterations, method=method),
                               dev32, dev8)
    # a second call on the same context reuses the scratch and gives the same bytes
    a = ctx.denoise(RGBA32F, d_guide.ptr)
    guarded = ctx.check_guards()[0]
    b = ctx.denoise(RGBA32F, d_guide.ptr)
    assert a.tobytes() == b.tobytes() and ctx.check_guards() == (guarded, 0)
    # nothing else changed: both images, the statistics, the fold records, the guide
    for img in (TRACE, ACCUM):
        assert ctx.read(img, native).tobytes() == before[img].tobytes(), img
    assert _stats_tuple(ctx.stats()) == stats
    after = ctx.fold_records(with_total=True)
    assert after[1] == records[1] and after[0].tobytes() == records[0].tobytes()
    assert d_guide.read().tobytes() == hits.tobytes()
    # ... and the frame loop goes on as if the filter had never run
    ctx.trace(case.push(4))
    ctx.accumulate(3)
    twin = case.context(mode=mode)
    for frame in range(4):
        twin.trace(case.push(1 + frame))
        twin.accumulate(frame)
    assert ctx.read(ACCUM, native).tobytes() == twin.read(ACCUM, native).tobytes()
    twin.close()
    ctx.close()
    for buf in (d_guide, dev32, dev8):
        buf.free()


def test_pipeline_mirrors():
    """RayTracePipeline.first_hits_into, DiffusePipeline.denoised and RenderPassOverFrame.render_denoised."""
    size = (37, 23)
    cam, settings = E.preset("box")
    settings.num_samples, settings.max_bounces = 1, 4
    ctx = E.HrtContext(size, device=0, mode=_lib.MODE_RGBA32F)
    pipe, diffuse = E.RayTracePipeline(ctx, size, settings), E.DiffusePipeline(ctx, size)
    for frame in range(2):
        pipe.compute(cam, frame)
        diffuse.next_frame(frame, pipe.image())
    d_guide = DevBuf(size[0] * size[1] * 32)
    pipe.first_hits_into(cam, d_guide.ptr)
    hits = d_guide.read().view(_lib.HIT_DTYPE).reshape(size[1], size[0])
    assert hits.tobytes() == pipe.first_hits(cam).tobytes()
    src = ctx.read(ACCUM, RGBA32F)
    got = diffuse.denoised(d_guide.ptr, RGBA32F, sigma_colour=2.0, iterations=4)
    assert equal(got, D.denoise(src, 4, (2.0,) + SIGMAS[1:], hits))
    assert equal(diffuse.denoised(), D.denoise(src, 5, SIGMAS, None, fmt_rgba8=True))
    target = DevBuf(size[0] * size[1] * 4)
    rp = E.RenderPassOverFrame(ctx, _lib.PRESENT_R8G8B8A8)
    pt = E.PresentTarget(target.ptr, target.nbytes, size[0], size[1], None, _lib.PRESENT_R8G8B8A8)
    ctx.present_wait(rp.render_denoised(diffuse.image(), pt, d_guide.ptr))
    want = present_ref.present_bytes(D.denoise(src, 5, SIGMAS, hits, fmt_rgba8=True), size[0], size[1], size[0] * 4,
                                     present_ref.R8G8B8A8, target.nbytes, 0, FILL)
    assert target.read().tobytes() == want.tobytes()
    ctx.close()
    d_guide.free()
    target.free()


# ---- 3. hrt_denoise_present ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_denoise_present(mode):
    size = w, h = (64, 36)
    native = RGBA8 if mode == _lib.MODE_RGBA8 else RGBA32F
    case = SceneCase("box", size, num_samples=1, max_bounces=4)
    ctx = case.context(mode=mode, debug=True)
    for frame in range(3):
        ctx.trace(case.push(1 + frame))
        ctx.accumulate(frame)
    d_guide = DevBuf(w * h * 32)
    ctx.intersect_primary_into(case.push(), d_guide.ptr)
    hits = d_guide.read().view(_lib.HIT_DTYPE).reshape(h, w)
    plain = DevBuf(w * h * 4)
    t0 = ctx.present(ACCUM, plain.ptr, plain.nbytes, w, h)
    shots = [  # image, target size, pitch padding, offset, byte order, guide, method
        (ACCUM, (w, h), 0, 0, _lib.PRESENT_B8G8R8A8, True, _lib.DENOISE_AUTO),
        (ACCUM, (w, h), 20, 16, _lib.PRESENT_R8G8B8A8, True, _lib.DENOISE_TILED),
        (TRACE, (w, h), 4, 4, _lib.PRESENT_B8G8R8A8, False, _lib.DENOISE_DIRECT),
        (ACCUM, (50, 31), 12, 0, _lib.PRESENT_R8G8B8A8, True, _lib.DENOISE_TILED),
        (TRACE, (97, 80), 0, 8, _lib.PRESENT_B8G8R8A8, True, _lib.DENOISE_AUTO),
    ]
    srcs = {img: ctx.read(img, native) for img in (TRACE, ACCUM)}
    targets, tickets = [], []
    for image, (wt, ht), pad, offset, order, guided, method in shots:
        pitch = wt * 4 + pad
        buf = DevBuf(offset + ht * pitch + 256)
        tickets.append(ctx.denoise_present(buf.ptr + offset, ht * pitch, wt, ht, pitch, order,
                                           d_guide.ptr if guided else None, image_id=image, method=method))
        filtered = D.denoise(srcs[image], 5, SIGMAS, hits if guided else None, fmt_rgba8=True)
        targets.append((buf, present_ref.present_bytes(filtered, wt, ht, pitch, order, buf.nbytes, offset, FILL)))
    # tickets continue hrt_present's sequence
    assert tickets == [t0 + 1 + i for i in range(len(shots))]
    t_next = ctx.present(ACCUM, plain.ptr, plain.nbytes, w, h)
    assert t_next == tickets[-1] + 1
    # work issued afterwards does not show in the targets
    ctx.trace(case.push(9))
    ctx.accumulate(3)
    ctx.present_wait(ctx.present(TRACE, plain.ptr, plain.nbytes, w, h))
    for t in tickets:
        assert ctx.present_done(t)
    for k, (buf, want) in enumerate(targets):
        assert buf.read().tobytes() == want.tobytes(), shots[k]
    assert ctx.read(ACCUM, native).tobytes() != srcs[ACCUM].tobytes()  # (the later frame did change the accumulator)
    ctx.synchronize()
    assert ctx.check_guards()[1] == 0
    ctx.close()
    for buf, _ in targets:
        buf.free()
    d_guide.free()
    plain.free()


# ---- 4. the rejections -------------------------------------------------------------------------------------------

def test_rejections_enqueue_nothing_and_leave_the_context_usable():
    size = w, h = (37, 23)
    case = SceneCase("box", size, num_samples=1, max_bounces=2)
    ctx = case.context()
    ctx.trace(case.push(1))
    ctx.accumulate(0)
    ctx.trace(case.push(2))
    ctx.accumulate(1)
    lib, handle = ctx.lib, ctx.handle
    d_guide = DevBuf(w * h * 32 + 16)
    ctx.intersect_primary_into(case.push(), d_guide.ptr)
    host = np.full(w * h * 16, FILL, np.uint8)
    target = DevBuf(w * h * 4)
    good = ctx.denoise_info()
    before = ctx.denoise(RGBA32F, d_guide.ptr)
    t0 = ctx.present(ACCUM, target.ptr, target.nbytes, w, h)
    ctx.present_wait(t0)
    shown = target.read()

    def raw(info=good, guide=d_guide.ptr, fmt=RGBA32F, dst=host.ctypes.data, nbytes=host.nbytes):
        return lib.hrt_denoise(handle, ctypes.byref(info) if info is not None else None, ctypes.c_void_p(guide or 0), fmt,
                               ctypes.c_void_p(dst or 0), nbytes)

    def raw_present(info=good, guide=d_guide.ptr, image=ACCUM, dst=target.ptr, nbytes=target.nbytes):
        pi, t = _lib.PresentInfo(image, _lib.PRESENT_B8G8R8A8, w, h, w * 4, 0), ctypes.c_uint64(99)
        st = lib.hrt_denoise_present(handle, ctypes.byref(info) if info is not None else None, ctypes.c_void_p(guide or 0),
                                     ctypes.byref(pi), ctypes.c_void_p(dst or 0), nbytes, ctypes.byref(t))
        assert t.value == 99
        return st

    def altered(**kw):
        info = ctx.denoise_info()
        for k, v in kw.items():
            setattr(info, k, v)
        return info

    bad_infos = [("iterations", 0), ("iterations", 6), ("flags", 1), ("method", 99), ("image_id", 2),
                 ("image_id", ACCUM | _lib.IMG_LOCAL)]
    bad_infos += [(s, v) for s in ("sigma_colour", "sigma_normal", "sigma_depth")
                  for v in (0.0, -1.0, float("nan"), float("inf"))]
    for call in (raw, raw_present):
        assert call(info=None) == 1 and b"null info" in lib.hrt_last_error(handle)
        for field, value in bad_infos:
            assert call(info=altered(**{field: value})) == 1, (field, value)
            assert b"hrt_denoise" in lib.hrt_last_error(handle)
        hits_host = np.zeros(w * h, dtype=_lib.HIT_DTYPE)
        assert call(guide=hits_host.ctypes.data) == 1 and b"guide" in lib.hrt_last_error(handle)   # host memory
        assert call(guide=d_guide.ptr + 8) == 1 and b"aligned" in lib.hrt_last_error(handle)        # misaligned
        assert call(dst=None) == 1
    assert raw(fmt=7) == 1 and b"format" in lib.hrt_last_error(handle)
    assert raw(nbytes=w * h * 16 - 1) == 1 and b"too small" in lib.hrt_last_error(handle)
    assert raw_present(nbytes=target.nbytes - 1) == 1
    assert raw_present(image=TRACE) == 1 and b"image_id" in lib.hrt_last_error(handle)  # differs from the filter's
    assert raw_present(dst=host.ctypes.data, nbytes=w * h * 4) == 1                     # pageable host target
    assert (host == FILL).all() and target.read().tobytes() == shown.tobytes()
    # nothing was enqueued or issued: the next ticket follows t0, and the context works as before
    assert ctx.present(ACCUM, target.ptr, target.nbytes, w, h) == t0 + 1
    assert ctx.denoise(RGBA32F, d_guide.ptr).tobytes() == before.tobytes()
    ctx.close()
    # a row-tile partition, with and without a communicator, and an unpartitioned context joined to one
    parts = [case.context(partition=(8, p, 2)) for p in range(2)]
    for joined in (False, True):
        if joined:
            E.HrtContext.comm_init_all(parts)
        for c in parts:
            with pytest.raises(_lib.HrtError, match="partition"):
                c.denoise(RGBA8)
            with pytest.raises(_lib.HrtError, match="partition"):
                c.denoise_present(target.ptr, target.nbytes, w, h)
    for c in parts:
        c.close()
    single = case.context()
    E.HrtContext.comm_init_all([single])
    with pytest.raises(_lib.HrtError, match="communicator"):
        single.denoise(RGBA8)
    single.close()
    d_guide.free()
    target.free()


# ---- 5. the C++ mirror ---------------------------------------------------------------------------------------------

def test_cpp_mirror_denoise(tmp_path):
    """include/hrt_app.hpp's first_hits_into / denoised / render_denoised (tests/cpp/denoise_demo) give the
    reference's bytes on the box scene's geometry."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "denoise_demo.mk"], check=True)  # (up to date after build())
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
    r = subprocess.run([os.path.join(cpp, "denoise_demo"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    w, h = 48, 32
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [w, h] and len(raw) == 8 + w * h * (16 + 4 + 4)
    guided = np.frombuffer(raw[8:8 + w * h * 16], F32).reshape(h, w, 4)
    plain = np.frombuffer(raw[8 + w * h * 16:8 + w * h * 20], np.uint8).reshape(h, w, 4)
    shown = np.frombuffer(raw[8 + w * h * 20:], np.uint8)
    # the demo's scene through the Python mirror: the same geometry, Lambertian grey, 1 sample, 4 bounces, light on
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    st = E.RayTracerSettings(num_samples=1, max_bounces=4, use_environment_lighting=True,
                             sphere_data=[E.Sphere(s.centre, s.radius, grey) for s in settings.sphere_data],
                             mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in settings.mesh_data])
    ctx = E.HrtContext((w, h), device=0)
    pipe, diffuse, cam = E.RayTracePipeline(ctx, (w, h), st), E.DiffusePipeline(ctx, (w, h)), E.Camera()
    for frame in range(3):
        pipe.compute(cam, frame)
        diffuse.next_frame(frame, pipe.image())
    acc, hits = ctx.read(ACCUM), pipe.first_hits(cam)
    ctx.close()
    assert equal(guided, D.denoise(acc, 5, SIGMAS, hits))
    assert equal(plain, D.denoise(acc, 5, SIGMAS, None, fmt_rgba8=True))
    want = present_ref.present_pixels(D.denoise(acc, 5, SIGMAS, hits, fmt_rgba8=True), w, h, present_ref.B8G8R8A8)
    assert shown.tobytes() == want.tobytes()
