"""Radiance queries on the device (hrt_radiance).  Every comparison is bitwise (a NaN
equals a NaN): the scan against the oracle's orc_trace_pixel on a 1 x 1 image (tests/radiance_ref.py), the two
hierarchy methods against the scan's bytes and counts under every option set of tests/test_gpu_intersect.py, a
whole frame against hrt_trace, shapes, refill and buffer bounds on the debug library, the edges of the push
block, non-interference with the frame loop, the argument errors, and the C++ mirror.

The batch per scene (radiance_ref.families, seeded): 1,280 camera pixels, 1,280 origins on random triangles
pushed off along the normal with random centres, 640 origins 1e3 / 1e6 scene diagonals away aimed at the scene,
640 records with seeds 0 and 0xFFFFFFFF, 80 irregular ones (NaN / inf origins, NaN / inf centres, a zero
centre) -- 3,920 queries at 3 samples and 4 bounces, run under the scene's push block with the environment
light on and again with it off.  The reference asserts, from the oracle alone, that a tenth of the batch
traces more segments than num_samples, that a tenth returns a nonzero rgb under the environment light, and
that the irregular queries trace segments: an all-zero or never-bouncing kernel cannot pass."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import radiance_ref as R
import test_gpu_intersect as TI
from helpers import E, SceneCase, _lib

pytestmark = pytest.mark.gpu

SEED = 26
SCAN, BVH, PAIRS, AUTO = TI.SCAN, TI.BVH, TI.PAIRS, _lib.QUERY_AUTO
METHODS = (SCAN, BVH, PAIRS)
SCENES = ["island", "cave", "degenerate", "ties", "spheres", "box"]
PER_FAMILY, SAMPLES, BOUNCES = 1280, 3, 4
CONFIGS = dict({"scan": (SCAN, {}, False)}, **TI.CONFIGS)


def counts(st):
    return int(st.scan_segments), int(st.segments), int(st.tri_tests)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The scene's batch and, per environment light setting (on, off): the oracle's rgba and the three counts.
    Read-only, shared by the cases below."""
    case, qs = TI.scene(name)
    base = R.copy_push(case.push(), num_samples=SAMPLES, max_bounces=BOUNCES)
    fam = R.families(case, qs, base, PER_FAMILY, SEED)
    queries = np.concatenate([fam[k] for k in ("camera", "surface", "far", "seeds", "irregular")])
    queries.setflags(write=False)
    irregular = R.always_irregular(queries)
    out = {}
    for light in (1, 0):
        pc = R.copy_push(base, use_environment_light=light)
        rgba, seg, tests = R.oracle(case, pc, queries)
        rgba.setflags(write=False)
        scan = int(seg[irregular].sum())
        print(f"{name} light {light}: {int((seg > SAMPLES).sum())} of {len(queries)} queries bounce, "
              f"{int((rgba[:, :3] != 0).any(1).sum())} nonzero, segments {int(seg.sum())}, scan segments {scan}")
        assert (seg > SAMPLES).sum() >= 0.1 * len(queries), name
        assert light == 0 or (rgba[:, :3] != 0).any(1).sum() >= 0.1 * len(queries), name
        assert scan > 0 and (rgba[:, 3] == 1.0).all()
        out[light] = (pc, rgba, (scan, int(seg.sum()), int(tests.sum())), seg)
    return queries, out


# ---- 1. SCAN equals the oracle; 2. BVH and PAIRS equal SCAN under every option set ------------------------------

@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", SCENES)
def test_radiance_equals_oracle(name, config):
    """config `scan`: the literal scan against the oracle, bytes, segments and tri_tests (and scan_segments by
    construction).  The others: the hierarchy methods against the same reference, which the scan case pins to
    the scan's own bytes and counts, with the method that was asked for having run."""
    method, options, debug = CONFIGS[config]
    case, _ = TI.scene(name)
    queries, ref = reference(name)
    ctx = case.context(options=options, debug=debug)
    built = ctx.scene_info()["bvh_built"] == 1
    assert built or name == "spheres"
    expect = method if built else SCAN
    if built and config == "pairs_leaf1" and not TI.pairs_fits(case, 1, 4):
        assert name in ("cave", "spheres")
        expect = BVH  # the node image does not fit the LDS: PAIRS runs as BVH
    probe = ctx.ray_queries(queries["origin"][:1], [[0.0, 0.0, 1.0]])
    if name == "spheres":  # (its hierarchy is the null mesh's one triangle: whatever hrt_intersect's plan says)
        expect = ctx.intersect(probe, None, method=method, with_stats=True)[1].method_ran
    auto_expect = ctx.intersect(probe, None, method=PAIRS, with_stats=True)[1].method_ran
    for light in (1, 0):
        pc, want, want_counts, _ = ref[light]
        got, st = ctx.radiance(queries, pc, method, with_stats=True)
        assert st.method_ran == expect and st.reserved == 0
        assert R.same_bits(got, want), (light, R.explain(got, want, queries))
        assert counts(st) == want_counts, light
        plain = ctx.radiance(queries, pc, method)  # stats = NULL: PAIRS runs its other instantiation
        assert R.same_bits(plain, want), (light, "no stats", R.explain(plain, want, queries))
    if config in ("scan", "pairs", "pairs_leaf1"):  # AUTO: PAIRS when it fits, else BVH, else SCAN
        pc, want, want_counts, _ = ref[1]
        got, st = ctx.radiance(queries, pc, AUTO, with_stats=True)
        assert st.method_ran == auto_expect and R.same_bits(got, want) and counts(st) == want_counts
    ctx.close()


# ---- 3. the frame ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["island", "cave", "box"])
def test_every_pixel_of_a_frame(name):
    """Every pixel of a 64 x 36 frame at 4 samples, 8 bounces as queries: hrt_trace's RGBA32F image and its
    hrt_stats' segments and tri_tests, by each method."""
    case = SceneCase(name, (64, 36), 4, 8)
    pc = case.push(7)
    ctx = case.context(mode=_lib.MODE_RGBA32F)
    ctx.reset_stats()
    ctx.trace(pc)
    st = ctx.stats()
    image = ctx.read(_lib.IMG_TRACE, _lib.FMT_RGBA32F).reshape(-1, 4)
    ids = np.arange(64 * 36)
    queries = R.pixel_queries(case, pc, ids % 64, ids // 64)
    assert st.segments > 4 * len(ids)
    for method in METHODS + (AUTO,):
        got, rst = ctx.radiance(queries, pc, method, with_stats=True)
        assert rst.method_ran == (PAIRS if method == AUTO else method)
        assert R.same_bits(got, image), (method, R.explain(got, image, queries))
        assert (rst.segments, rst.tri_tests, rst.scan_segments) == (st.segments, st.tri_tests, 0), method
    after = ctx.stats()
    assert (after.segments, after.tri_tests) == (st.segments, st.tri_tests)  # hrt_stats untouched
    ctx.close()


def test_pipeline_radiance_pixels():
    """RayTracePipeline.radiance_pixels: the bytes `compute` stores at the listed pixels."""
    case, _ = TI.scene("box")
    W, H = case.size
    ctx = E.HrtContext(case.size, device=0, mode=_lib.MODE_RGBA32F)
    pipe = E.RayTracePipeline(ctx, case.size, case.settings)
    pipe.num_samples, pipe.max_bounces = 3, 4
    pipe.compute(case.camera, 5)
    image = ctx.read(_lib.IMG_TRACE, _lib.FMT_RGBA32F)
    rng = np.random.default_rng(SEED)
    xs, ys = rng.integers(0, W, 300), rng.integers(0, H, 300)
    got = pipe.radiance_pixels(case.camera, xs, ys, 5)
    assert got.shape == (300, 4) and R.same_bits(got, image[ys, xs])
    assert (got[:, :3] != 0).any()
    with pytest.raises(ValueError):
        pipe.radiance_pixels(case.camera, [W], [0], 5)
    ctx.close()


# ---- 4. shapes, refill and bounds (debug library: guard bands around every device buffer) ------------------------

SHAPES = [1, 63, 64, 65, 257, 1000, TI.CHUNK + 77]


@pytest.mark.parametrize("method", METHODS)
def test_shapes_and_bounds(method):
    """n around the wave and block sizes and above the staging chunk, host and device buffers: exactly n results
    are written, what lies past them keeps its sentinel, and no guard band is touched."""
    case, _ = TI.scene("box")
    pool, ref = reference("box")
    pc, pool_want, _, _ = ref[1]
    order = np.resize(np.arange(len(pool)), SHAPES[-1])
    queries, want = pool[order], pool_want[order]
    ctx = case.context(debug=True)
    pad = 3
    for n in SHAPES:
        host = np.full((n + pad, 4), -7.0, np.float32)
        st = ctx.radiance_into(pc, queries.ctypes.data, n, host.ctypes.data, method, with_stats=True)
        assert st.method_ran == method and st.segments >= n * SAMPLES
        assert R.same_bits(host[:n], want[:n]), (n, R.explain(host[:n], want[:n], queries[:n]))
        assert (host[n:] == -7.0).all(), n
        d_q, d_out = TI.DevBuf(n * 32).write(queries[:n]), TI.DevBuf((n + pad) * 16)
        ctx.radiance_into(pc, d_q.ptr, n, d_out.ptr, method)
        got = d_out.read()
        assert R.same_bits(got[:n * 16].view(np.float32).reshape(-1, 4), want[:n]) and (got[n * 16:] == 0xA5).all(), n
        if n <= 1000:  # host queries into device results, device queries into host results
            d_out2 = TI.DevBuf((n + pad) * 16)
            ctx.radiance_into(pc, queries.ctypes.data, n, d_out2.ptr, method)
            got = d_out2.read()
            assert R.same_bits(got[:n * 16].view(np.float32).reshape(-1, 4), want[:n]) and (got[n * 16:] == 0xA5).all(), n
            host = np.full((n + pad, 4), -7.0, np.float32)
            ctx.radiance_into(pc, d_q.ptr, n, host.ctypes.data, method)
            assert R.same_bits(host[:n], want[:n]) and (host[n:] == -7.0).all(), n
            d_out2.free()
        d_q.free()
        d_out.free()
    buffers, corrupted = ctx.check_guards()
    assert buffers > 0 and corrupted == 0
    # device pointers off their 16-byte alignment
    d_q, d_out = TI.DevBuf(64 * 32).write(queries[:64]), TI.DevBuf(64 * 16)
    for qp, op in ((d_q.ptr, d_out.ptr + 4), (queries.ctypes.data, d_out.ptr + 8), (d_q.ptr + 4, d_out.ptr)):
        with pytest.raises(_lib.HrtError) as e:
            ctx.radiance_into(pc, qp, 33, op, method)
        assert e.value.status == 1
    assert (d_out.read() == 0xA5).all()
    d_q.free()
    d_out.free()
    ctx.close()


@pytest.mark.parametrize("name", ["box", "cave"])
def test_permuted_and_skewed_batches(name):
    """A query's answer does not depend on its place or its company: a permuted batch gives the permuted
    output, and a batch whose first 64-blocks are all sky misses and whose later ones are the scene's longest
    paths gives each query's solo answer (the lanes of the early blocks refill from the late ones)."""
    case, _ = TI.scene(name)
    pool, ref = reference(name)
    pc, want, _, seg = ref[1]
    rng = np.random.default_rng([SEED, 4])
    perm = rng.permutation(len(pool))
    by_len = np.argsort(seg, kind="stable")
    misses, longest = by_len[seg[by_len] == SAMPLES], by_len[::-1][:640]
    assert len(misses) >= 64 and seg[longest].min() > SAMPLES
    skew = np.concatenate([np.resize(misses, 64 * 40), longest])
    ctx = case.context()
    for method in METHODS:
        got = ctx.radiance(pool[perm], pc, method)
        assert R.same_bits(got, want[perm]), (method, R.explain(got, want[perm], pool[perm]))
        got, st = ctx.radiance(pool[skew], pc, method, with_stats=True)
        assert R.same_bits(got, want[skew]), (method, R.explain(got, want[skew], pool[skew]))
        assert st.segments == int(seg[skew].sum())
    ctx.close()


# ---- 5. edges of the push block, against the oracle ----------------------------------------------------------------

EDGES = {
    "samples_0": dict(num_samples=0),
    "samples_neg": dict(num_samples=-1),
    "bounces_0": dict(max_bounces=0),
    "bounces_neg": dict(max_bounces=-1),
    "fixed_direction": dict(jitter_size=0.0),  # with an identity matrix: centre is the direction
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_edges(edge):
    case, _ = TI.scene("box")
    pool, ref = reference("box")
    queries = pool[::8].copy()
    pc = R.copy_push(ref[1][0], **EDGES[edge])
    if edge == "fixed_direction":
        for k in range(16):
            pc.cam_alignment_mat[k] = 1.0 if k % 5 == 0 else 0.0
    want, seg, tests = R.oracle(case, pc, queries)
    if edge == "samples_0":
        assert np.isnan(want[:, :3]).all() and seg.sum() == 0
    if edge == "samples_neg":
        assert (want[:, :3] == 0).all() and seg.sum() == 0
    if edge == "bounces_neg":
        assert (want[:, :3] == 0).all() and seg.sum() == 0
    if edge == "bounces_0":
        assert (seg == SAMPLES).all() and (want[:, :3] != 0).any()
    if edge == "fixed_direction":
        assert (seg > SAMPLES).any() and (want[:, :3] != 0).any()
    ctx = case.context()
    for method in METHODS:
        got, st = ctx.radiance(queries, pc, method, with_stats=True)
        assert st.method_ran == method
        assert R.same_bits(got, want), (method, R.explain(got, want, queries))
        assert (st.segments, st.tri_tests) == (int(seg.sum()), int(tests.sum())), method
    ctx.close()


# ---- 6. non-interference ---------------------------------------------------------------------------------------------

def _frame_loop(case, queries, pc, query):
    """test_gpu_intersect._frame_loop's calls with hrt_radiance calls of each method between every pair."""
    ctx = case.context(options={_lib.OPT_FOLD_RECORDS: 1})
    W, H = case.size
    target = TI.DevBuf(W * H * 4)
    d_q, d_out = TI.DevBuf(queries.nbytes).write(queries), TI.DevBuf(16 * len(queries))
    answers = []

    def ask():
        if query:
            for method in METHODS:
                answers.append(ctx.radiance(queries, pc, method).tobytes())
            ctx.radiance_into(pc, d_q.ptr, len(queries), d_out.ptr, PAIRS, with_stats=True)

    out = []
    ask()
    for k in range(4):
        ctx.trace(case.push(k))
        ask()
        ctx.accumulate(k)
        ask()
    out += [ctx.read(_lib.IMG_TRACE).tobytes(), ctx.read(_lib.IMG_ACCUM).tobytes(), TI._stats_tuple(ctx.stats())]
    ask()
    tickets = [ctx.present(_lib.IMG_ACCUM, target.ptr, target.nbytes, W, H)]
    ask()
    ctx.compute_n(case.push(4), 4)
    ask()
    tickets.append(ctx.present(_lib.IMG_ACCUM, target.ptr, target.nbytes, W, H))
    ask()
    ctx.present_wait(tickets[-1])
    recs, total = ctx.fold_records(with_total=True)
    out += [ctx.read(_lib.IMG_TRACE).tobytes(), ctx.read(_lib.IMG_ACCUM).tobytes(), TI._stats_tuple(ctx.stats()),
            recs.tobytes(), total, tickets, target.read().tobytes()]
    for buf in (target, d_q, d_out):
        buf.free()
    ctx.close()
    return out, answers


def test_radiance_queries_do_not_disturb_the_frame_loop():
    case = SceneCase("island", (64, 36), 2, 4)
    pc = R.copy_push(case.push(), num_samples=SAMPLES, max_bounces=BOUNCES)
    p = np.random.default_rng(SEED).integers(0, 64 * 36, 900)
    queries = R.pixel_queries(case, pc, p % 64, p // 64)
    (plain, _), (mixed, answers) = _frame_loop(case, queries, pc, False), _frame_loop(case, queries, pc, True)
    names = ("trace image", "accumulator", "hrt_stats", "trace image after compute_n", "accumulator after compute_n",
             "hrt_stats after compute_n", "fold records", "fold record total", "present tickets", "presented bytes")
    for what, a, b in zip(names, plain, mixed):
        assert a == b, (what, a, b) if "hrt_stats" in what else what
    assert plain[7] >= 4 and plain[8][0] < plain[8][1]
    # ... and the frame loop does not disturb the queries
    assert len(answers) == 3 * 13 and len(set(answers)) == 1
    rgba = np.frombuffer(answers[0], np.float32).reshape(-1, 4)
    assert (rgba[:, :3] != 0).any() and (rgba[:, 3] == 1).all()


# ---- 7. errors and empties -------------------------------------------------------------------------------------------

def test_errors_and_empty_calls():
    case, _ = TI.scene("box")
    pool, ref = reference("box")
    pc, want, _, _ = ref[1]
    queries = pool[:100].copy()
    out = np.full((100, 4), -7.0, np.float32)
    bare = E.HrtContext(case.size, device=0)
    with pytest.raises(_lib.HrtError) as e:
        bare.radiance(queries, pc, SCAN)
    assert e.value.status == 4  # HRT_ERR_NO_SCENE
    bare.close()
    ctx = case.context()
    st = _lib.RadianceStats(9, 9, 9, 9, 9)
    call = ctx.lib.hrt_radiance
    args = (ctx.handle, ctypes.byref(pc), _lib.ptr(queries), 100)
    for bad_method in (4, 99, 0xFFFFFFFF):
        assert call(*args, bad_method, _lib.ptr(out), ctypes.byref(st)) == 1
    for field, value in (("init", 1), ("num_meshes", len(case.meshes) + 1), ("num_spheres", -1)):
        assert call(ctx.handle, ctypes.byref(R.copy_push(pc, **{field: value})), _lib.ptr(queries), 100, SCAN,
                    _lib.ptr(out), ctypes.byref(st)) == 1, field
    assert call(ctx.handle, None, _lib.ptr(queries), 100, SCAN, _lib.ptr(out), ctypes.byref(st)) == 1
    assert call(ctx.handle, ctypes.byref(pc), None, 4, SCAN, _lib.ptr(out), ctypes.byref(st)) == 1  # NULL queries, n > 0
    assert call(*args, SCAN, None, ctypes.byref(st)) == 1                                          # NULL rgba, n > 0
    assert (out == -7.0).all() and (st.method_ran, st.scan_segments, st.segments, st.tri_tests) == (9, 9, 9, 9)
    # empty calls: OK, nothing written, the statistics filled
    assert call(ctx.handle, ctypes.byref(pc), None, 0, AUTO, None, ctypes.byref(st)) == 0
    assert (st.method_ran, st.reserved) + counts(st) == (PAIRS, 0, 0, 0, 0)
    assert call(ctx.handle, ctypes.byref(pc), _lib.ptr(queries), 0, BVH, _lib.ptr(out), ctypes.byref(st)) == 0
    assert st.method_ran == BVH and (out == -7.0).all()
    assert call(ctx.handle, ctypes.byref(pc), None, 0, SCAN, None, None) == 0
    assert ctx.radiance(queries[:0], pc).shape == (0, 4)
    # the image size, camera position and rng_offset of pc are ignored
    other = R.copy_push(pc, width=3, height=5, num_rays=1, rng_offset=99)
    other.cam_pos[0] = 1e9
    for method in METHODS + (AUTO,):
        got = ctx.radiance(queries, other, method)
        assert R.same_bits(got, want[:100]), method
    ctx.close()


class DeviceTensor:
    """What HrtContext.radiance reads of a torch device tensor of n x 8 words: shape and data_ptr()."""

    def __init__(self, records):
        self.buf = TI.DevBuf(records.nbytes).write(records)
        self.shape = (len(records), 8)

    def data_ptr(self):
        return self.buf.ptr


def test_device_tensor_queries():
    case, _ = TI.scene("box")
    pool, ref = reference("box")
    pc, want, _, _ = ref[1]
    ctx = case.context()
    t = DeviceTensor(pool[:500])
    for method in METHODS:
        assert R.same_bits(ctx.radiance(t, pc, method), want[:500]), method
    t.buf.free()
    ctx.close()


# ---- 8. the C++ mirror ---------------------------------------------------------------------------------------------------

def test_cpp_mirror_radiance(tmp_path):
    """include/hrt_app.hpp's RayTracePipeline::radiance / radiance_pixels (tests/cpp/radiance_demo) give the
    Python mirror's bytes on the box scene's geometry."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "radiance_demo.mk"], check=True)  # (up to date after build())
    case, _ = TI.scene("box")
    pool, _ = reference("box")
    queries = np.ascontiguousarray(pool[:1000])
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        f.write(np.uint32(len(case.settings.sphere_data)).tobytes())
        for s in case.settings.sphere_data:
            f.write(np.float32([*s.centre, s.radius]).tobytes())
        f.write(np.uint32(len(case.settings.mesh_data)).tobytes())
        for m in case.settings.mesh_data:
            f.write(np.uint32([len(m.mesh.positions), len(m.mesh.indices)]).tobytes())
            f.write(m.mesh.positions.tobytes())
            f.write(m.mesh.indices.tobytes())
        f.write(np.uint32(len(queries)).tobytes())
        f.write(queries.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([os.path.join(cpp, "radiance_demo"), str(src), str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    n, npix = len(queries), 16 * 16
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [n, npix] and len(raw) == 8 + 16 * (n + npix)
    got = np.frombuffer(raw[8:], np.float32).reshape(-1, 4)
    # the demo's scene: the same geometry, every primitive Lambertian grey, 3 samples, 4 bounces, light on
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    st = E.RayTracerSettings(num_samples=3, max_bounces=4, use_environment_lighting=True,
                             sphere_data=[E.Sphere(s.centre, s.radius, grey) for s in case.settings.sphere_data],
                             mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in case.settings.mesh_data])
    ctx = E.HrtContext((16, 16), device=0)
    pipe = E.RayTracePipeline(ctx, (16, 16), st)
    cam = E.Camera()
    want = ctx.radiance(queries, pipe.push_constants(cam, 0, False))
    ids = np.arange(npix)
    want_px = pipe.radiance_pixels(cam, ids % 16, ids // 16, 3)
    ctx.close()
    assert (want[:, :3] != 0).any()
    assert R.same_bits(got[:n], want), R.explain(got[:n], want, queries)
    assert R.same_bits(got[n:], want_px)
