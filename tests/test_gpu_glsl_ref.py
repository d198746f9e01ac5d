"""The HIP kernels against the reference's own shader text (MI355X; DESIGN.md 2 "Parity status").

The expected values come from oracle/_ref/libglslref.so -- assets/raytracing.glsl and assets/image_combiner.glsl of the
reference, translated mechanically and compiled against oracle/glsl_ref/glsl_shim.hpp -- computed on the host in the
test, with the oracle no longer in between: hrt_trace's texels, floats and triangle-test counts by six kernels, and
hrt_radiance, hrt_intersect and hrt_accumulate / hrt_compute_n by each of their methods.  Every comparison is bitwise (a
NaN equals a NaN).  The library is built where a reference checkout exists and travels with the tree; without it the
tests skip."""
import functools

import numpy as np
import pytest

import glsl_ref_cases as G
import pyoracle
import radiance_ref as R
from helpers import _lib, mismatch_report
from image_ref import same_floats

GLSL = pyoracle.load_glsl_ref()
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(GLSL is None, reason="no reference checkout and no built oracle/_ref/libglslref.so")]

F32 = np.float32
FLT_MAX = F32(3.402823466e+38)
# the literal kernel, AUTO, BUNDLE_CULL_LDS, BUNDLE_WQ, BUNDLE_WQ_L2 and the per-lane hierarchy; every one of them
# promises the exact triangle-test count (tests/test_gpu_parity.py, tests/test_gpu_wq_l2.py)
KERNELS = {"literal": _lib.KERNEL_LITERAL, "auto": _lib.KERNEL_AUTO, "cull_lds": _lib.KERNEL_BUNDLE_CULL_LDS,
           "wq": _lib.KERNEL_BUNDLE_WQ, "wq_l2": _lib.KERNEL_BUNDLE_WQ_L2, "bvh": _lib.KERNEL_BUNDLE_BVH}
FRAMES = {"box": ((45, 33), 3, 6), "spheres": ((40, 30), 2, 8), "island": ((96, 64), 4, 8), "cave": ((64, 48), 2, 8),
          "ties": ((36, 28), 3, 8), "degenerate": ((48, 36), 3, 8)}
METHODS = {"scan": _lib.QUERY_SCAN, "bvh": _lib.QUERY_BVH, "pairs": _lib.QUERY_PAIRS}


@functools.lru_cache(maxsize=None)
def shader_frame(name, rng_offset=1):
    """(case, the shader's texels, stored floats and triangle-buffer reads): computed once, read-only."""
    size, spp, bounces = FRAMES[name]
    case = G.scene_case(name, size, spp, bounces, rng_offset)
    g8, g32, tests = pyoracle.glsl_trace(case.push(), case.rays, case.spheres, case.tris, case.meshes)
    g8.setflags(write=False)
    g32.setflags(write=False)
    return case, g8, g32, tests


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", list(FRAMES))
def test_trace_equals_the_shader(name, kernel):
    """hrt_trace: HRT_MODE_RGBA8's bytes against the shader's texels, HRT_MODE_RGBA32F's floats against what the
    shader handed to imageStore, and hrt_stats.tri_tests against the shader's reads of its triangle buffer."""
    case, g8, g32, tests = shader_frame(name)
    for mode, fmt, want in ((_lib.MODE_RGBA8, _lib.FMT_RGBA8, g8), (_lib.MODE_RGBA32F, _lib.FMT_RGBA32F, g32)):
        ctx = case.context(mode=mode, variant=KERNELS[kernel])
        ctx.trace(case.push())
        st = ctx.stats()
        img = ctx.read(_lib.IMG_TRACE, fmt)
        ctx.close()
        if fmt == _lib.FMT_RGBA8:
            assert np.array_equal(img, want), mismatch_report(img, want)
        else:
            same = same_floats(img, want)
            assert same.all(), f"{int((~same).any(-1).sum())} pixels differ"
        assert st.tri_tests == tests


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("name", ["island", "box", "spheres"])
def test_radiance_equals_the_shader_pixels(name, method):
    """hrt_radiance on a permuted subset of a frame's pixels against the shader's main() at those pixels: the vec4
    before quantisation, and the triangle tests of exactly those pixels."""
    case, _, _, _ = shader_frame(name)
    W, H = case.size
    pc = case.push()
    ids = np.random.default_rng(31).permutation(W * H)[:600]
    xs, ys = ids % W, ids // W
    want, _, tests = pyoracle.glsl_trace_pixels(pc, case.rays, case.spheres, case.tris, case.meshes, xs, ys)
    ctx = case.context()
    got, st = ctx.radiance(R.pixel_queries(case, pc, xs, ys), pc, METHODS[method], with_stats=True)
    ctx.close()
    assert same_floats(got, want).all(), int((~same_floats(got, want)).any(-1).sum())
    assert st.tri_tests == int(tests.sum())


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("name", ["island", "cave"])
def test_intersect_equals_the_shader_world_hit(name, method):
    """hrt_intersect on bounce-like rays against the shader's world_hit: kind, t and normal.  The ray's direction is
    normalised as S11 says (the shim's normalize, S4) before the shader sees it; a hit is a sphere's when world_hit
    over the spheres alone returns the same distance (spheres are scanned first and win ties)."""
    case = G.scene_case(name, (16, 12), 1, 1)
    n = 3000
    o, d = G.bounce_like_rays(case, np.random.default_rng(37), n)
    unit_d = np.zeros((n, 3), F32)
    pyoracle.batch(GLSL, "glr_shim_op", 2, n, d, None, None, unit_d)
    pc = case.push()
    full, alone, reads = np.zeros((n, 19), F32), np.zeros((n, 19), F32), np.zeros(1, np.uint64)
    pyoracle.batch(GLSL, "glr_world_hit", n, pc, case.spheres if len(case.spheres) else None, case.tris, case.meshes,
                   o, unit_d, full, reads)
    pc.num_meshes = 0
    pyoracle.batch(GLSL, "glr_world_hit", n, pc, case.spheres if len(case.spheres) else None, None, None, o, unit_d,
                   alone, None)
    hit = full[:, 6] < FLT_MAX
    sphere = hit & (alone[:, 6] == full[:, 6])
    kind = np.where(sphere, _lib.HIT_SPHERE, np.where(hit, _lib.HIT_TRIANGLE, _lib.HIT_MISS))
    assert 0.2 * n < hit.sum() < n
    ctx = case.context()
    hits, st = ctx.intersect(o, d, method=METHODS[method], with_stats=True)
    ctx.close()
    assert np.array_equal(hits["kind"], kind)
    assert same_floats(hits["t"], full[:, 6]).all()
    assert same_floats(hits["normal"], full[:, :3]).all()
    assert st.tri_tests == int(reads[0])


@pytest.mark.parametrize("how", ["accumulate", "compute_n"])
def test_progressive_rgba8_equals_the_shader_combiner(how):
    """Four progressive frames in RGBA8 -- the clear at frame 0, then frames 1..3 traced with rng_offset = frame --
    by hrt_trace + hrt_accumulate and by hrt_compute_n, against the shader's combiner fed with the shader's frames."""
    case = shader_frame("box")[0]
    args = (case.rays, case.spheres, case.tris, case.meshes)
    want = np.full(case.size[::-1] + (4,), 77, np.uint8)
    pyoracle.glsl_combine_rgba8(0, want, pyoracle.glsl_trace(case.push(init=True), *args)[0])
    for k in (1, 2, 3):
        pyoracle.glsl_combine_rgba8(k, want, pyoracle.glsl_trace(case.push(k), *args)[0])
    ctx = case.context()
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    if how == "accumulate":
        for k in (1, 2, 3):
            ctx.trace(case.push(k))
            ctx.accumulate(k)
    else:
        ctx.compute_n(case.push(1), 3)
    got = ctx.read(_lib.IMG_ACCUM)
    ctx.close()
    assert np.array_equal(got, want), mismatch_report(got, want)
