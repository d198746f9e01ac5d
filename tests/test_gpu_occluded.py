"""Occlusion queries on the device (hrt_occluded), every comparison bitwise against
hrt_intersect on the same rays: occluded(i) == (hit(i).kind != 0), by the scan, by the per-lane traversal and
by the pair traversal under every option set of tests/test_gpu_intersect.py; t_max at a hit's exact t and its
two neighbours (where a traversal seeded with t_max can go wrong by one ulp); surface-to-surface segments as
RayTracePipeline.visible builds them; shapes and buffer bounds on the debug library; non-interference with the
frame loop; the argument errors; the C++ mirror.

Ray families: tests/query_ref.py's (a)-(i) as test_gpu_intersect.scan_reference builds them, at 2,048 rays per
family and 32,768 of family (i) (a quarter of that file's sizes: every case here creates a context, runs
hrt_intersect and hrt_occluded and stays within a few seconds).  Each scene's batch must hold both answers on at
least a tenth of its rays by the scan's own hrt_intersect result, so an all-zero or all-one kernel cannot pass.
Sphere-only scenes have no triangles to aim families (c), (d) and (i) at and go without them."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import query_ref as Q
import test_gpu_intersect as TI
from helpers import E, _lib

pytestmark = pytest.mark.gpu

SEED = TI.SEED
SCAN, BVH, PAIRS = TI.SCAN, TI.BVH, TI.PAIRS
METHODS = (SCAN, BVH, PAIRS)
PER_FAMILY, FAR_GRAZING = 2048, 1 << 15
SCENES = ["island", "cave", "degenerate", "ties", "spheres", "box"]
CONFIGS = dict({"scan": (SCAN, {}, False)}, **TI.CONFIGS)


def pack(flags):
    """bool[n] -> the ceil(n / 32) words hrt_occluded writes: ray i is bit i & 31 of word i >> 5, tail bits 0."""
    b = np.packbits(np.asarray(flags, bool), bitorder="little")
    return np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)]).view(np.uint32)


def explain(got, want, rays):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if bad.size == 0:
        return "identical"
    k = int(bad[0])
    return f"{bad.size} of {len(want)} bits differ; first at ray {k} {rays[k]}: got {int(got[k])}, want {int(want[k])}"


@functools.lru_cache(maxsize=None)
def reference(name):
    """The scene's rays, hrt_intersect(SCAN)'s kind != 0 for each, and its tri_tests and scan_rays."""
    case, qs = TI.scene(name)
    ctx = case.context()
    has_tris = len(case.meshes) > 0
    rays, _ = TI.families(name, PER_FAMILY, ctx, "abcdefgh" if has_tris else "abefgh")
    if has_tris:
        rays = np.concatenate([rays, Q.family(qs, "i", FAR_GRAZING, SEED)])
    hits, st = ctx.intersect(rays, None, method=SCAN, with_stats=True)
    ctx.close()
    want = hits["kind"] != 0
    want.setflags(write=False)
    assert st.method_ran == SCAN and st.scan_rays == Q.count_irregular(rays) > 0
    # both answers on at least a tenth of the batch, by the reference alone
    assert 0.1 * len(rays) <= int(want.sum()) <= 0.9 * len(rays), (name, int(want.sum()), len(rays))
    return rays, want, st.tri_tests, st.scan_rays


# ---- 1. equals hrt_intersect ---------------------------------------------------------------------------------

@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", SCENES)
def test_occluded_equals_intersect(name, config):
    method, options, debug = CONFIGS[config]
    case, _ = TI.scene(name)
    rays, want, tri_tests, scan_rays = reference(name)
    ctx = case.context(options=options, debug=debug)
    built = ctx.scene_info()["bvh_built"] == 1
    assert built or name == "spheres"
    expect = method if built else SCAN
    if built and config == "pairs_leaf1" and not TI.pairs_fits(case, 1, 4):
        # cave's node image at leaves of one triangle does not fit the LDS: PAIRS runs as BVH
        assert name in ("cave", "spheres")
        expect = BVH
    hits, hst = ctx.intersect(rays, None, method=method, with_stats=True)
    if name == "spheres":  # (its hierarchy is the null mesh's one triangle: whatever hrt_intersect's plan says)
        expect = hst.method_ran
    bits, st = ctx.occluded(rays, method, with_stats=True)
    words, st2 = ctx.occluded(rays, method, with_stats=True, packed=True)
    ctx.close()
    print(f"{name} {config}: {int(want.sum())} of {len(rays)} occluded, tri_tests {st.tri_tests}, scan_rays {st.scan_rays}")
    assert st.method_ran == hst.method_ran == expect
    assert (st.scan_rays, st.tri_tests) == (hst.scan_rays, hst.tri_tests) == (scan_rays, tri_tests)
    assert bits.dtype == np.bool_ and bits.shape == (len(rays),)
    assert np.array_equal(hits["kind"] != 0, want)
    assert np.array_equal(bits, want), explain(bits, want, rays)
    assert words.tobytes() == pack(want).tobytes()
    assert st.occluded == st2.occluded == int(want.sum()) == sum(bin(int(w)).count("1") for w in words)


# ---- 2. t_max at the hit -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["island", "cave", "degenerate", "spheres", "box"])
def test_t_max_at_the_hit(name):
    """Rays that hit at t, with t_max = t, the next float up and the next float down: 0, 1, 0, by every method."""
    case, qs = TI.scene(name)
    ctx = case.context()
    first = np.concatenate([Q.family(qs, f, PER_FAMILY, SEED + 9, case.push()) for f in "ab"])
    hits = ctx.intersect(first, None, method=SCAN)
    sel = np.flatnonzero(hits["kind"] != 0)
    assert len(sel) >= 256
    rays, t = first[sel], hits["t"][sel].astype(np.float32)
    assert ((t > 0.001) & (t < Q.FLT_MAX)).all()
    batch, want = [], []
    for t_max, answer in ((t, False), (np.nextafter(t, np.float32(np.inf)), True), (np.nextafter(t, np.float32(0)), False)):
        r = rays.copy()
        r["t_max"] = t_max
        batch.append(r)
        want.append(np.full(len(r), answer))
    batch, want = np.concatenate(batch), np.concatenate(want)
    assert np.array_equal(ctx.intersect(batch, None, method=SCAN)["kind"] != 0, want)  # the definition agrees
    for method in METHODS:
        got, st = ctx.occluded(batch, method, with_stats=True)
        assert st.method_ran == ctx.intersect(batch[:1], None, method=method, with_stats=True)[1].method_ran
        assert np.array_equal(got, want), (method, explain(got, want, batch))
        assert st.occluded == len(rays)
    ctx.close()


# ---- 3. segments ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["island", "cave"])
def test_segments(name):
    """4,096 point pairs on random triangles, as RayTracePipeline.visible builds their rays, at t_max = |b - a|
    and at t_max scaled by 1 - 2^-20 and 1 + 2^-20 (just short of the far surface, and just through it)."""
    case, qs = TI.scene(name)
    rng = np.random.default_rng([SEED, 77])
    _, a = Q._tri_points(qs, rng, 4096)
    _, b = Q._tri_points(qs, rng, 4096)
    seg = E.RayTracePipeline.segment_rays(a, b)
    d = b.astype(np.float32) - a.astype(np.float32)
    assert np.array_equal(seg["origin"], a.astype(np.float32)) and np.array_equal(seg["direction"], d)
    sq = d * d
    assert np.array_equal(seg["t_max"], np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2], dtype=np.float32))
    batch = []
    for scale in (1.0, 1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20):
        r = seg.copy()
        r["t_max"] = seg["t_max"] * np.float32(scale)
        batch.append(r)
    batch = np.concatenate(batch)
    ctx = E.HrtContext(case.size, device=0)
    pipe = E.RayTracePipeline(ctx, case.size, case.settings)
    want = ctx.intersect(batch, None, method=SCAN)["kind"] != 0
    blocked = int(want[:4096].sum())
    print(f"{name}: {blocked} of 4096 segments blocked; scaled down {int(want[4096:8192].sum())}, up {int(want[8192:].sum())}")
    assert 0 < blocked < 4096  # both visible and blocked pairs
    for method in METHODS:
        hits, hst = ctx.intersect(batch, None, method=method, with_stats=True)
        got, st = ctx.occluded(batch, method, with_stats=True)
        assert st.method_ran == hst.method_ran == method
        assert np.array_equal(hits["kind"] != 0, want)
        assert np.array_equal(got, want), (method, explain(got, want, batch))
        assert (st.tri_tests, st.scan_rays, st.occluded) == (hst.tri_tests, hst.scan_rays, int(want.sum()))
        vis = pipe.visible(a, b, method)
        assert vis.dtype == np.bool_ and np.array_equal(vis, ~want[:4096]), method
    assert np.array_equal(pipe.visible(a, b), ~want[:4096])
    ctx.close()


# ---- 4. shapes and bounds (debug library: guard bands around every device buffer) -----------------------------

SHAPES = [1, 31, 32, 33, 63, 64, 65, 257, 1000, TI.CHUNK + 77]


@pytest.mark.parametrize("method", METHODS)
def test_shapes_and_bounds(method):
    """n around the word, wave and block sizes and above the staging chunk, host and device buffers: exactly
    ceil(n / 32) words are written, the tail bits of the last one are 0, the words past them keep their
    sentinel, and no guard band (the bits staging buffer's among them) is touched."""
    case, _ = TI.scene("box")
    ctx = case.context(debug=True)
    pool, _ = TI.families("box", 2048, ctx, "abcdefh")
    rays = np.resize(pool, SHAPES[-1])
    want = ctx.intersect(rays, None, method=SCAN)["kind"] != 0
    assert 0.1 * len(want) < want.sum() < 0.9 * len(want)
    pad = 4
    for n in SHAPES:
        nw = (n + 31) // 32
        words = pack(want[:n])
        assert len(words) == nw and (n % 32 == 0 or words[-1] >> (n % 32) == 0)
        host = np.full(nw + pad, 0xCDCDCDCD, np.uint32)
        st = ctx.occluded_into(rays.ctypes.data, n, host.ctypes.data, method, with_stats=True)
        assert st.method_ran == method and st.occluded == int(want[:n].sum())
        assert host[:nw].tobytes() == words.tobytes(), n
        assert (host[nw:] == 0xCDCDCDCD).all(), n
        d_rays, d_bits = TI.DevBuf(n * 32).write(rays[:n]), TI.DevBuf((nw + pad) * 4)
        st = ctx.occluded_into(d_rays.ptr, n, d_bits.ptr, method, with_stats=True)
        got = d_bits.read()
        assert st.occluded == int(want[:n].sum())
        assert got[:nw * 4].tobytes() == words.tobytes() and (got[nw * 4:] == 0xA5).all(), n
        # host rays into device bits, device rays into host bits
        d_bits2 = TI.DevBuf((nw + pad) * 4)
        ctx.occluded_into(rays.ctypes.data, n, d_bits2.ptr, method)
        got = d_bits2.read()
        assert got[:nw * 4].tobytes() == words.tobytes() and (got[nw * 4:] == 0xA5).all(), n
        host = np.full(nw + pad, 0xCDCDCDCD, np.uint32)
        ctx.occluded_into(d_rays.ptr, n, host.ctypes.data, method)
        assert host[:nw].tobytes() == words.tobytes() and (host[nw:] == 0xCDCDCDCD).all(), n
        for buf in (d_rays, d_bits, d_bits2):
            buf.free()
    buffers, corrupted = ctx.check_guards()
    assert buffers > 0 and corrupted == 0
    # a device bits pointer off its 4-byte alignment, device rays off their 16 bytes
    d_rays, d_bits = TI.DevBuf(64 * 32).write(rays[:64]), TI.DevBuf(64)
    for rp, bp in ((d_rays.ptr, d_bits.ptr + 2), (rays.ctypes.data, d_bits.ptr + 2), (d_rays.ptr + 4, d_bits.ptr)):
        with pytest.raises(_lib.HrtError) as e:
            ctx.occluded_into(rp, 33, bp, method)
        assert e.value.status == 1
    assert (d_bits.read() == 0xA5).all()
    d_rays.free()
    d_bits.free()
    ctx.close()


# ---- 5. non-interference -------------------------------------------------------------------------------------

def _frame_loop(case, rays, query):
    """test_gpu_intersect._frame_loop with hrt_occluded calls of each method between every pair of calls."""
    ctx = case.context(options={_lib.OPT_FOLD_RECORDS: 1})
    W, H = case.size
    target = TI.DevBuf(W * H * 4)
    d_rays, d_bits = TI.DevBuf(rays.nbytes).write(rays), TI.DevBuf(4 * ((len(rays) + 31) // 32))
    answers = []

    def ask():
        if query:
            for method in METHODS:
                answers.append(ctx.occluded(rays, method).tobytes())
            ctx.occluded_into(d_rays.ptr, len(rays), d_bits.ptr, PAIRS)

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
    for buf in (target, d_rays, d_bits):
        buf.free()
    ctx.close()
    return out, answers


def test_occlusion_queries_do_not_disturb_the_frame_loop():
    case = TI.SceneCase("island", (64, 36), 2, 4)
    qs = Q.QueryScene(case)
    rays = np.concatenate([Q.family(qs, f, 300, SEED, case.push()) for f in "abfh"])
    (plain, _), (mixed, answers) = _frame_loop(case, rays, False), _frame_loop(case, rays, True)
    names = ("trace image", "accumulator", "hrt_stats", "trace image after compute_n", "accumulator after compute_n",
             "hrt_stats after compute_n", "fold records", "fold record total", "present tickets", "presented bytes")
    for what, a, b in zip(names, plain, mixed):
        assert a == b, (what, a, b) if "hrt_stats" in what else what
    assert plain[7] >= 4 and plain[8][0] < plain[8][1]
    # ... and the frame loop does not disturb the queries: every call gave the same bits, both answers among them
    assert len(answers) == 3 * 13 and len(set(answers)) == 1
    bits = np.frombuffer(answers[0], np.bool_)
    assert 0 < bits.sum() < len(bits)


# ---- 6. errors and empties -----------------------------------------------------------------------------------

def test_errors_and_empty_calls():
    case, qs = TI.scene("box")
    rays = Q.family(qs, "b", 100, SEED)
    bits = np.full(4, 0xCDCDCDCD, np.uint32)
    bare = E.HrtContext(case.size, device=0)
    with pytest.raises(_lib.HrtError) as e:
        bare.occluded(rays, SCAN)
    assert e.value.status == 4  # HRT_ERR_NO_SCENE
    bare.close()
    ctx = case.context()
    for bad_method in (4, 99, 0xFFFFFFFF):
        with pytest.raises(_lib.HrtError) as e:
            ctx.occluded(rays, bad_method)
        assert e.value.status == 1
    st = _lib.OcclusionStats(9, 9, 9, 9, 9)
    assert ctx.lib.hrt_occluded(ctx.handle, None, 4, SCAN, _lib.ptr(bits), ctypes.byref(st)) == 1   # NULL rays, n > 0
    assert ctx.lib.hrt_occluded(ctx.handle, _lib.ptr(rays), 4, SCAN, None, ctypes.byref(st)) == 1   # NULL bits, n > 0
    assert (bits == 0xCDCDCDCD).all() and (st.method_ran, st.scan_rays, st.tri_tests, st.occluded) == (9, 9, 9, 9)
    # empty calls: OK, nothing written, the statistics filled
    assert ctx.lib.hrt_occluded(ctx.handle, None, 0, _lib.QUERY_AUTO, None, ctypes.byref(st)) == 0
    assert (st.method_ran, st.reserved, st.scan_rays, st.tri_tests, st.occluded) == (BVH, 0, 0, 0, 0)
    assert ctx.lib.hrt_occluded(ctx.handle, _lib.ptr(rays), 0, PAIRS, _lib.ptr(bits), ctypes.byref(st)) == 0
    assert st.method_ran == PAIRS and (bits == 0xCDCDCDCD).all()
    assert ctx.lib.hrt_occluded(ctx.handle, None, 0, SCAN, None, None) == 0
    empty = ctx.occluded(rays[:0])
    assert empty.shape == (0,) and empty.dtype == np.bool_ and ctx.occluded(rays[:0], packed=True).shape == (0,)
    # AUTO: BVH on a built hierarchy; the same bits by every method, with or without statistics
    want = ctx.intersect(rays, None, method=SCAN)["kind"] != 0
    assert 0 < want.sum() < len(want)
    got, st = ctx.occluded(rays, with_stats=True)
    assert st.method_ran == BVH and np.array_equal(got, want)
    for method in METHODS:
        assert np.array_equal(ctx.occluded(rays, method), want)
    ctx.close()


class DeviceTensor:
    """What HrtContext.occluded reads of a torch device tensor of n x 8 float32: shape and data_ptr().  (The
    tensor itself would cost this suite torch's import and its GPU start-up, some twelve seconds.)"""

    def __init__(self, rays):
        self.buf = TI.DevBuf(rays.nbytes).write(rays)
        self.shape = (len(rays), 8)

    def data_ptr(self):
        return self.buf.ptr


def test_device_tensor_rays():
    case, qs = TI.scene("box")
    rays = Q.family(qs, "b", 100, SEED)
    ctx = case.context()
    want = ctx.intersect(rays, None, method=SCAN)["kind"] != 0
    t = DeviceTensor(rays)
    for method in METHODS:
        assert np.array_equal(ctx.occluded(t, method), want)
    words, st = ctx.occluded(t, PAIRS, with_stats=True, packed=True)
    assert words.tobytes() == pack(want).tobytes() and st.occluded == int(want.sum())
    t.buf.free()
    ctx.close()


# ---- 7. the C++ mirror -----------------------------------------------------------------------------------------

def test_cpp_mirror_visible_and_occluded(tmp_path):
    """include/hrt_app.hpp's RayTracePipeline::visible / occluded (tests/cpp/occlusion_demo) give the Python
    mirror's answers on the box scene."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "occlusion_demo.mk"], check=True)  # (up to date after build())
    case, qs = TI.scene("box")
    rng = np.random.default_rng([SEED, 78])
    n = 1000
    a = Q._tri_points(qs, rng, n)[1].astype(np.float32)
    b = Q._tri_points(qs, rng, n)[1].astype(np.float32)
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
        f.write(np.uint32(n).tobytes())
        f.write(a.tobytes())
        f.write(b.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([os.path.join(cpp, "occlusion_demo"), str(src), str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    assert np.frombuffer(raw[:4], np.uint32)[0] == n and len(raw) == 4 + 2 * n
    got = np.frombuffer(raw[4:], np.uint8).astype(bool)
    ctx = E.HrtContext((16, 16), device=0)
    pipe = E.RayTracePipeline(ctx, (16, 16), case.settings)
    vis = pipe.visible(a, b)
    unbounded = E.RayTracePipeline.segment_rays(a, b)
    unbounded["t_max"] = Q.FLT_MAX
    occ = ctx.occluded(unbounded)
    ctx.close()
    assert 0 < vis.sum() < n and 0 < occ.sum()
    assert np.array_equal(got[:n], vis) and np.array_equal(got[n:], occ)
