"""Ray queries on the device (hrt_intersect / hrt_intersect_primary), every comparison
bitwise: the literal scan against a world_hit built from the oracle's own intersecting_aabb /
intersecting_tri (tests/query_ref.py), the two hierarchy traversals against the scan on rays aimed where
their conservative bounds are weakest, the primary variant, shapes and buffer bounds on the debug library,
non-interference with the frame loop, and the argument errors.

Ray families (query_ref.family, all seeded): (a) pixel-centre rays, (b) origin on a random triangle and a
random direction, (c) origin and direction in a triangle's plane, and rays just outside the grazing band
aimed at a triangle's edge from up to 1e3 scene diagonals away, (d) aimed at a vertex or an edge midpoint,
(e) axis directions and directions with zero components, (f) origins 1e3 / 1e6 scene diagonals away and at
the scene-box centre, (g) t_max at a first pass's exact t and its two neighbours, (h) non-finite origins,
zero / underflowing / overflowing directions, NaN / negative / tiny t_max, (i) near-band rays from 1e4 / 1e5 scene
diagonals aimed just off a triangle's edge (case 2 only: the rays that need the node margins' b R term)."""
import ctypes
import functools

import numpy as np
import pytest

import query_ref as Q
from helpers import E, SceneCase, _lib

pytestmark = pytest.mark.gpu

SEED = 20
SCAN, BVH, PAIRS = _lib.QUERY_SCAN, _lib.QUERY_BVH, _lib.QUERY_PAIRS
LDS_BYTES = 160 * 1024 - 64  # the pair traversal's dynamic LDS (hrt_kernels.hip kMaxLdsScene)
FAR_GRAZING = 1 << 17  # rays of family (i) in case 2: about one in 5,000 of them sees the node margins' b R term


# ---- scenes ----------------------------------------------------------------------------------------------

def tie_soup(seed=5, n=24):
    """The tie soup of tests/test_gpu_parity.py at a size the Python reference can scan: a triangle soup stored
    twice in one mesh and again as a second mesh (exact ties inside and across meshes), plus a sphere."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-4, 4, (n, 3))
    v = np.concatenate([a[:, None, :], (a + rng.uniform(-1.5, 1.5, (n, 3)))[:, None, :],
                        (a + rng.uniform(-1.5, 1.5, (n, 3)))[:, None, :]], 1).reshape(-1, 3)
    v = np.concatenate([v, v]).astype(np.float32)
    idx = np.arange(len(v), dtype=np.uint32)
    st = E.RayTracerSettings(num_samples=1, max_bounces=1, use_environment_lighting=True,
                             sphere_data=[E.Sphere([0.0, 0.0, 0.0], 1.0, E.MetalMaterial([0.9, 0.9, 0.9], 1.0, 0.0))],
                             mesh_data=[E.RayTracingMesh(E.Mesh(v, idx), E.LambertianMaterial([0.8, 0.7, 0.6])),
                                        E.RayTracingMesh(E.Mesh(v.copy(), idx.copy()), E.MetalMaterial([0.6, 0.7, 0.9], 0.8, 0.1))])
    return SceneCase(settings=st, camera=E.Camera([0.3, 0.2, -9.0], [0.0, 0.0, 1.0]), size=(72, 56))


def degenerate():
    """The degenerate-geometry scene of tests/test_gpu_parity.py: slivers, zero-area triangles, triangles nearly
    edge-on to the view, an exact duplicate, a huge and a tiny triangle, an opposite-winding copy of it all as a
    second mesh, and a sphere tying with a triangle."""
    rng = np.random.default_rng(11)
    tris = []
    for _ in range(200):
        a = rng.uniform(-3, 3, 3)
        b = a + rng.uniform(-2, 2, 3)
        tris += [a, b, a + (b - a) * rng.uniform(0, 1) + rng.normal(size=3) * 1e-6]
    for _ in range(50):
        a = rng.uniform(-3, 3, 3)
        tris += [a, a, a + rng.uniform(-1, 1, 3)]
    for _ in range(100):
        a = rng.uniform(-3, 3, 3)
        tris += [a, a + np.array([2.0, 0.0, 1e-5]), a + np.array([0.0, 0.0, 2.0])]
    base = np.array([[-2.0, -2.0, 1.0], [2.0, -2.0, 1.0], [0.0, 2.0, 1.0]])
    tris += list(base) + list(base)
    tris += [np.array([-1e6, -1e6, 50.0]), np.array([1e6, -1e6, 50.0]), np.array([0.0, 1e6, 50.0])]
    tris += [np.array([0.0, 0.0, 2.0]), np.array([1e-30, 0.0, 2.0]), np.array([0.0, 1e-30, 2.0])]
    v = np.array(tris, np.float32)
    idx = np.arange(len(v), dtype=np.uint32)
    st = E.RayTracerSettings(num_samples=1, max_bounces=1, use_environment_lighting=True,
                             sphere_data=[E.Sphere([0.0, 0.0, 1.0], 0.5, E.MetalMaterial([0.9, 0.9, 0.9], 1.0, 0.0))],
                             mesh_data=[E.RayTracingMesh(E.Mesh(v, idx), E.LambertianMaterial([0.8, 0.7, 0.6])),
                                        E.RayTracingMesh(E.Mesh(v[::-1].copy(), idx.copy()),
                                                         E.MetalMaterial([0.6, 0.7, 0.9], 0.8, 0.1))])
    return SceneCase(settings=st, camera=E.Camera([0.1, 0.2, -6.0], [0.0, 0.0, 1.0]), size=(64, 48))


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "ties":
        case = tie_soup()
    elif name == "degenerate":
        case = degenerate()
    else:
        case = SceneCase(name, {"box": (37, 23)}.get(name, (64, 36)), 1, 1)
    return case, Q.QueryScene(case)


def families(name, n, ctx, letters="abcdefgh"):
    """n rays of each listed family for the scene, in letter order; (g) from a SCAN pass over (a) and (b)."""
    case, qs = scene(name)
    out = {}
    for f in letters:
        if f != "g":
            out[f] = Q.family(qs, f, n, SEED, case.push())
    if "g" in letters:
        first = np.concatenate([Q.family(qs, f, n, SEED + 9, case.push()) for f in "ab"])
        out["g"] = Q.t_max_family(first, ctx.intersect(first, None, method=SCAN), n, SEED)
        assert len(out["g"]) == n
    return np.concatenate([out[f] for f in letters]), out


def explain(got, want, rays):
    bad = np.flatnonzero((np.ascontiguousarray(got).view(np.uint32).reshape(-1, 8) !=
                          np.ascontiguousarray(want).view(np.uint32).reshape(-1, 8)).any(1))
    if bad.size == 0:
        return "identical"
    k = int(bad[0])
    return f"{bad.size} of {len(got)} hits differ; first at ray {k} {rays[k]}: got {got[k]}, want {want[k]}"


def same(got, want, rays):
    assert got.tobytes() == want.tobytes(), explain(got, want, rays)


# ---- 1. SCAN equals the oracle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box", "spheres", "ties", "island"])
def test_scan_equals_oracle(name):
    """Every field of every hit, and the triangle-test and scan-fallback counts, against query_ref.world_hit."""
    case, qs = scene(name)
    ctx = case.context()
    if name == "island":  # 64 rays over (a)-(g): the reference scans 1,610 triangles per ray here
        rays, _ = families(name, 10, ctx, "abcdefg")
        rays = rays[:64]
    else:
        rays, _ = families(name, 256, ctx, "abefgh" if name == "spheres" else "abcdefgh")
    hits, st = ctx.intersect(rays, None, method=SCAN, with_stats=True)
    ctx.close()
    before = qs.oracle_calls
    want, tests, scans = qs.hits(rays)
    assert qs.oracle_calls - before <= 250_000
    same(hits, want, rays)
    assert (st.method_ran, st.tri_tests, st.scan_rays) == (SCAN, tests, scans)
    kinds = np.bincount(want["kind"], minlength=3)
    assert kinds[0] > 0 and (kinds[1] > 0 or len(case.spheres) == 0) and (kinds[2] > 0 or len(case.meshes) == 0), kinds


# ---- 2. the hierarchy methods equal SCAN -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scan_reference(name):
    """The scene's 8 x 8,192 rays of families (a)-(h) and 131,072 of family (i), their SCAN hits and statistics,
    and the rays among them that were constructed non-finite (S11's scan fallback)."""
    case, _ = scene(name)
    ctx = case.context()
    rays, fam = families(name, 8192, ctx)
    rays = np.concatenate([rays, Q.family(scene(name)[1], "i", FAR_GRAZING, SEED)])
    hits, st = ctx.intersect(rays, None, method=SCAN, with_stats=True)
    ctx.close()
    irregular = Q.count_irregular(rays)  # family (h)'s, and in-plane directions along a degenerate triangle's edges
    assert (st.method_ran, st.scan_rays) == (SCAN, irregular) and 0 < Q.count_irregular(fam["h"]) <= irregular < 8192
    return rays, hits, st.tri_tests, irregular


def pairs_fits(case, leaf, width):
    """Whether the pair traversal's node image and stacks fit the LDS for this hierarchy (hrt_kernels.hip
    wq_stack_cap, restated): else HRT_QUERY_PAIRS is specified to run as BVH."""
    img = np.zeros(70000 * 12, np.float32)
    n = _lib.load().hrt_debug_bvh_wq_nodes(case.tris.ctypes.data, len(case.tris), case.meshes.ctypes.data,
                                           len(case.meshes), leaf, width, img.ctypes.data, img.size)
    return n > 0 and n * 48 + 16 * (512 + 4 * (64 * (1 + 2 * leaf) + 128)) <= LDS_BYTES


CONFIGS = {
    "bvh": (BVH, {}, False),
    "pairs": (PAIRS, {}, False),
    "pairs_radius1": (PAIRS, {_lib.OPT_WQ_NODE_RADIUS: 1}, False),
    "pairs_radius2": (PAIRS, {_lib.OPT_WQ_NODE_RADIUS: 2}, False),
    "pairs_node_cap128": (PAIRS, {_lib.OPT_WQ_NODE_CAP: 128}, False),
    "pairs_tri_cap128": (PAIRS, {_lib.DEBUG_OPT_WQ_TRI_CAP: 128}, True),
    "pairs_width2": (PAIRS, {_lib.OPT_BVH_WIDTH: 2}, False),
    "pairs_width4": (PAIRS, {_lib.OPT_BVH_WIDTH: 4}, False),
    "pairs_leaf1": (PAIRS, {_lib.OPT_BVH_LEAF_SIZE: 1}, False),
    "pairs_leaf4": (PAIRS, {_lib.OPT_BVH_LEAF_SIZE: 4}, False),
}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ["island", "cave", "degenerate"])
def test_hierarchy_equals_scan(name, config):
    """BVH and PAIRS give SCAN's bytes on 8,192 rays of each family (and 131,072 of family (i)), with the method that was asked for having
    run (no fallback hiding a traversal that never ran) on exactly the rays that are not family (h)'s
    non-finite ones."""
    method, options, debug = CONFIGS[config]
    case, _ = scene(name)
    rays, want, tri_tests, irregular = scan_reference(name)
    ctx = case.context(options=options, debug=debug)
    assert ctx.scene_info()["bvh_built"] == 1
    expect = method
    if config == "pairs_leaf1" and not pairs_fits(case, 1, 4):
        # leaves of one triangle double the node image: cave's (3,815 nodes, 183 KB) does not fit the LDS and
        # PAIRS is specified to run as BVH there; island's and the degenerate scene's fit
        assert name == "cave"
        expect = BVH
    hits, st = ctx.intersect(rays, None, method=method, with_stats=True)
    ctx.close()
    assert st.method_ran == expect
    assert st.scan_rays == irregular
    assert st.tri_tests == tri_tests
    same(hits, want, rays)


# ---- 3. primary rays ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box", "island"])
def test_primary_equals_intersect(name):
    case, qs = scene(name)
    W, H = case.size
    pc = case.push()
    ctx = case.context()
    ys, xs = np.divmod(np.arange(W * H), W)
    rays = Q.primary_rays(case, pc, xs, ys)
    whole = {}
    for method in (SCAN, BVH, PAIRS):
        img, st = ctx.intersect_primary(pc, method=method, with_stats=True)
        assert img.shape == (H, W) and st.method_ran == method and st.scan_rays == 0
        same(img.reshape(-1), ctx.intersect(rays, None, method=method), rays)
        whole[method] = img
    assert whole[SCAN].tobytes() == whole[BVH].tobytes() == whole[PAIRS].tobytes()
    img = whole[SCAN]
    assert (img["kind"] == 2).any()
    if name == "box":
        want, tests, _ = qs.hits(rays)
        same(img.reshape(-1), want, rays)
        assert ctx.intersect_primary(pc, method=SCAN, with_stats=True)[1].tri_tests == tests
        # the push block's counts, not the uploaded ones (S11): no sphere and the first three of the seven meshes
        fewer = case.push()
        fewer.num_spheres, fewer.num_meshes = 0, 3
        want, tests, _ = qs.hits(rays, n_spheres=0, n_meshes=3)
        assert (want["kind"] == 2).any() and want["mesh"][want["kind"] == 2].max() <= 2 and not (want["kind"] == 1).any()
        assert want.tobytes() != img.tobytes()
        for method in (SCAN, BVH, PAIRS):
            got, st = ctx.intersect_primary(fewer, method=method, with_stats=True)
            same(got.reshape(-1), want, rays)
            assert (st.method_ran, st.tri_tests) == (method, tests)
    # a pick at each corner, a ragged rectangle
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        for method in (SCAN, BVH, PAIRS):
            one = ctx.intersect_primary(pc, (x, y, 1, 1), method)
            assert one.shape == (1, 1) and one.tobytes() == img[y:y + 1, x:x + 1].tobytes(), (x, y, method)
    x0, y0, w, h = 5, 3, 17, 11
    for method in (SCAN, BVH, PAIRS):
        part = ctx.intersect_primary(pc, (x0, y0, w, h), method)
        assert part.tobytes() == np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w]).tobytes(), method
    ctx.close()
    # every part of a row-tile partition holds all ray centres: the same bytes from either part
    for part_index in (0, 1):
        part = case.context(partition=(8, part_index, 2))
        for method in (SCAN, PAIRS):
            assert part.intersect_primary(pc, method=method).tobytes() == img.tobytes(), (part_index, method)
        part.close()


def test_pick_and_first_hits():
    """RayTracePipeline.pick / first_hits on the cube scene: the centre pixel sees the cube's top face (mesh 0).
    (An even-sized image: the centre pixel of an odd-sized one lies on the optical axis, which is tangent to the
    scene's unit sphere at the face's centre -- there the reference's own scan answers the sphere.)"""
    camera, settings = E.preset("cube")
    W, H = 64, 64
    ctx = E.HrtContext((W, H), device=0)
    pipe = E.RayTracePipeline(ctx, (W, H), settings)
    hit = pipe.pick(camera, W // 2, H // 2)
    assert (int(hit["kind"]), int(hit["mesh"])) == (2, 0) and 0.001 < hit["t"] < Q.FLT_MAX
    assert hit["normal"].tolist() == [0.0, 1.0, 0.0] and hit["index"] < 12
    case = SceneCase("cube", (W, H), 1, 1)
    ray = Q.primary_rays(case, pipe.push_constants(camera, 0, False), [W // 2], [H // 2])
    assert hit.tobytes() == Q.QueryScene(case).hits(ray)[0][0].tobytes()
    first = pipe.first_hits(camera)
    assert first.shape == (H, W) and first[H // 2, W // 2].tobytes() == hit.tobytes()
    assert {0, 2} == set(np.unique(first["kind"]).tolist())  # sky and the cube (its sphere is inside it)
    assert pipe.first_hits(camera, (3, 2, 5, 4)).tobytes() == np.ascontiguousarray(first[2:6, 3:8]).tobytes()
    ctx.close()


def test_cpp_mirror_pick_and_first_hits(tmp_path):
    """include/hrt_app.hpp's RayTracePipeline::first_hits / pick (tests/cpp/pick_demo) give the Python mirror's
    records on the demo scene of tests/cpp/app_demo.cpp."""
    import os
    import subprocess

    from test_cpp_app import demo_settings
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "pick_demo.mk"], check=True)  # (up to date after build())
    W, H = 48, 30
    out = tmp_path / "pick.bin"
    r = subprocess.run([os.path.join(cpp, "pick_demo"), str(out), str(W), str(H)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [W, H] and len(raw) == 8 + (W * H + 2) * 32
    got = np.frombuffer(raw[8:], _lib.HIT_DTYPE)
    cam = E.Camera(position=(0.0, 0.3, 1.5), direction=(0.0, -0.1, -1.0))
    ctx = E.HrtContext((W, H), device=0)
    pipe = E.RayTracePipeline(ctx, (W, H), demo_settings(1, 1))
    first = pipe.first_hits(cam)
    assert got[:W * H].tobytes() == first.tobytes()
    assert got[W * H].tobytes() == pipe.pick(cam, W // 2, H // 2).tobytes() == first[H // 2, W // 2].tobytes()
    assert got[W * H + 1].tobytes() == pipe.pick(cam, 0, 0).tobytes()
    assert {1, 2} <= set(np.unique(first["kind"]).tolist())  # the spheres and the quad are in view
    ctx.close()


# ---- 4. shapes and bounds (debug library: guard bands around every device buffer) ---------------------

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
    def __init__(self, nbytes, fill=0xA5):
        p = ctypes.c_void_p()
        assert hip().hipMalloc(ctypes.byref(p), nbytes) == 0
        self.ptr, self.nbytes = int(p.value), nbytes
        assert hip().hipMemset(self.ptr, fill, nbytes) == 0 and hip().hipDeviceSynchronize() == 0

    def write(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes and hip().hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0
        return self

    def read(self):
        out = np.empty(self.nbytes, np.uint8)
        assert hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return out

    def free(self):
        hip().hipFree(self.ptr)


CHUNK = 1 << 16  # hrt_api.cpp kQueryChunk: host-side rays and hits are staged in chunks of this many records
SHAPES = [1, 63, 64, 65, 257, 1000, CHUNK + 77]


@pytest.mark.parametrize("method", [SCAN, BVH, PAIRS])
def test_shapes_and_bounds(method):
    """n around the wave and block sizes and above the staging chunk, host and device buffers: the first n
    records are the full batch's, the bytes past them keep their sentinel, and no guard band is touched."""
    case, qs = scene("box")
    ctx = case.context(debug=True)
    pool, _ = families("box", 2048, ctx, "abcdefh")
    rays = np.resize(pool, SHAPES[-1])
    want = ctx.intersect(rays, None, method=SCAN)
    pad = 4
    for n in SHAPES:
        host = np.full((n + pad) * 32, 0xCD, np.uint8)
        st = ctx.intersect_into(rays.ctypes.data, n, host.ctypes.data, method, with_stats=True)
        assert st.method_ran == method
        assert host[:n * 32].tobytes() == want[:n].tobytes(), (n, explain(host[:n * 32].view(_lib.HIT_DTYPE), want[:n], rays))
        assert (host[n * 32:] == 0xCD).all(), n
        d_rays, d_hits = DevBuf(n * 32).write(rays[:n]), DevBuf((n + pad) * 32)
        ctx.intersect_into(d_rays.ptr, n, d_hits.ptr, method)
        got = d_hits.read()
        assert got[:n * 32].tobytes() == want[:n].tobytes() and (got[n * 32:] == 0xA5).all(), n
        d_rays.free()
        d_hits.free()
    W, H = case.size
    full = ctx.intersect_primary(case.push(), method=method)
    d_hits = DevBuf((W * H + pad) * 32)
    st = _lib.QueryStats()
    ctx._check(ctx.lib.hrt_intersect_primary(ctx.handle, ctypes.byref(case.push()), 0, 0, W, H, method,
                                             ctypes.c_void_p(d_hits.ptr), ctypes.byref(st)), "hrt_intersect_primary")
    got = d_hits.read()
    assert got[:W * H * 32].tobytes() == full.tobytes() and (got[W * H * 32:] == 0xA5).all()
    d_hits.free()
    buffers, corrupted = ctx.check_guards()
    assert buffers > 0 and corrupted == 0
    ctx.close()


# ---- 5. non-interference -----------------------------------------------------------------------------------

def _stats_tuple(st):
    """hrt_stats without its timings and without wave_steps: that one sums, per work item, the item's longest
    lane, so it depends on how the planner split the tiles into items -- on the previous trace's measured tile
    costs and on whether another lane's trace was still running at launch (HRT_OPT_BUSY_SPLIT).  It differs
    between two runs of the same loop without any query (744 / 750 on one machine in one sitting; 950 when the
    blocking queries let every trace find the GPU idle); the header calls it comparable between launches of the
    same shape only, and tests/test_gpu_parity.py leaves it out for the same reason."""
    return (st.segments, st.tri_tests, st.traces, st.accumulates, st.last_kernel, st.last_block, st.last_frames)


def _frame_loop(case, rays, query):
    """A 4-frame realtime loop and a 4-frame hrt_compute_n with fold records and a present after each, with a
    query of each method between every pair of calls when `query`."""
    ctx = case.context(options={_lib.OPT_FOLD_RECORDS: 1})
    W, H = case.size
    target = DevBuf(W * H * 4)

    def ask():
        if query:
            for method in (SCAN, BVH, PAIRS):
                ctx.intersect(rays, None, method=method)
            ctx.intersect_primary(case.push(), (1, 1, 9, 7), PAIRS)

    out = []
    ask()
    for k in range(4):
        ctx.trace(case.push(k))
        ask()
        ctx.accumulate(k)
        ask()
    out += [ctx.read(_lib.IMG_TRACE).tobytes(), ctx.read(_lib.IMG_ACCUM).tobytes(), _stats_tuple(ctx.stats())]
    ask()
    tickets = [ctx.present(_lib.IMG_ACCUM, target.ptr, target.nbytes, W, H)]
    ask()
    ctx.compute_n(case.push(4), 4)
    ask()
    tickets.append(ctx.present(_lib.IMG_ACCUM, target.ptr, target.nbytes, W, H))
    ask()
    ctx.present_wait(tickets[-1])
    recs, total = ctx.fold_records(with_total=True)
    out += [ctx.read(_lib.IMG_TRACE).tobytes(), ctx.read(_lib.IMG_ACCUM).tobytes(), _stats_tuple(ctx.stats()),
            recs.tobytes(), total, tickets, target.read().tobytes()]
    target.free()
    ctx.close()
    return out


def test_queries_do_not_disturb_the_frame_loop():
    case = SceneCase("island", (64, 36), 2, 4)
    qs = Q.QueryScene(case)
    rays = np.concatenate([Q.family(qs, f, 300, SEED, case.push()) for f in "abfh"])
    plain, mixed = _frame_loop(case, rays, False), _frame_loop(case, rays, True)
    names = ("trace image", "accumulator", "hrt_stats", "trace image after compute_n", "accumulator after compute_n",
             "hrt_stats after compute_n", "fold records", "fold record total", "present tickets", "presented bytes")
    for what, a, b in zip(names, plain, mixed):
        assert a == b, (what, a, b) if "hrt_stats" in what else what
    assert plain[7] >= 4 and plain[8][0] < plain[8][1]


# ---- 6. errors ------------------------------------------------------------------------------------------------

def test_errors_and_empty_calls():
    case, qs = scene("box")
    rays = Q.family(qs, "b", 100, SEED)
    bare = E.HrtContext(case.size, device=0)
    with pytest.raises(_lib.HrtError) as e:
        bare.intersect(rays, None, method=SCAN)
    assert e.value.status == 4  # HRT_ERR_NO_SCENE
    with pytest.raises(_lib.HrtError) as e:
        bare.intersect_primary(case.push(), (0, 0, 1, 1))
    assert e.value.status == 4
    bare.close()
    ctx = case.context()
    W, H = case.size
    for bad_method in (4, 99, 0xFFFFFFFF):
        with pytest.raises(_lib.HrtError) as e:
            ctx.intersect(rays, None, method=bad_method)
        assert e.value.status == 1
        with pytest.raises(_lib.HrtError) as e:
            ctx.intersect_primary(case.push(), (0, 0, 1, 1), bad_method)
        assert e.value.status == 1
    for rect in ((W, 0, 1, 1), (0, H, 1, 1), (W - 1, 0, 2, 1), (0, H - 1, 1, 2), (0, 0, W + 1, 1), (0xFFFFFFFF, 0, 2, 1)):
        with pytest.raises(_lib.HrtError) as e:
            ctx.intersect_primary(case.push(), rect)
        assert e.value.status == 1, rect
    wrong = case.push()
    wrong.width += 1
    with pytest.raises(_lib.HrtError) as e:
        ctx.intersect_primary(wrong, (0, 0, 1, 1))
    assert e.value.status == 1
    over = case.push()
    over.num_meshes += 1
    with pytest.raises(_lib.HrtError) as e:
        ctx.intersect_primary(over, (0, 0, 1, 1))
    assert e.value.status == 1
    hits = np.zeros(4, _lib.HIT_DTYPE)
    assert ctx.lib.hrt_intersect(ctx.handle, None, 4, SCAN, _lib.ptr(hits), None) == 1       # NULL rays, n > 0
    assert ctx.lib.hrt_intersect(ctx.handle, _lib.ptr(rays), 4, SCAN, None, None) == 1       # NULL hits, n > 0
    assert ctx.lib.hrt_intersect_primary(ctx.handle, ctypes.byref(case.push()), 0, 0, 1, 1, SCAN, None, None) == 1
    # empty calls: OK, nothing done
    st = _lib.QueryStats(9, 9, 9, 9)
    assert ctx.lib.hrt_intersect(ctx.handle, None, 0, _lib.QUERY_AUTO, None, ctypes.byref(st)) == 0
    assert (st.method_ran, st.scan_rays, st.tri_tests) == (BVH, 0, 0)
    assert ctx.intersect(rays[:0], None).shape == (0,)
    assert ctx.intersect_primary(case.push(), (3, 3, 0, 5)).size == 0
    assert ctx.intersect_primary(case.push(), (W, H, 0, 0)).size == 0
    # AUTO: BVH on a built hierarchy, SCAN without one
    assert ctx.intersect(rays, None, with_stats=True)[1].method_ran == BVH
    # ... above 64 meshes the hierarchy is not built: every method runs (and says it ran) SCAN
    rng = np.random.default_rng(5)
    meshes = []
    for _ in range(70):
        v = (rng.uniform(-4, 4, 3) + rng.uniform(-1, 1, (3, 3))).astype(np.float32)
        meshes.append(E.RayTracingMesh(E.Mesh(v, np.arange(3, dtype=np.uint32)), E.LambertianMaterial([0.5, 0.5, 0.5])))
    many = SceneCase(settings=E.RayTracerSettings(num_samples=1, max_bounces=1, use_environment_lighting=True,
                                                  mesh_data=meshes),
                     camera=E.Camera([0.0, 0.0, -12.0], [0.0, 0.0, 1.0]), size=(16, 16))
    mctx = many.context()
    assert mctx.scene_info()["bvh_built"] == 0
    mrays = np.concatenate([Q.family(Q.QueryScene(many), f, 200, SEED, many.push()) for f in "abd"])
    mwant = mctx.intersect(mrays, None, method=SCAN)
    assert (mwant["kind"] == 2).any() and mwant["mesh"][mwant["kind"] == 2].max() > 63
    for method in (_lib.QUERY_AUTO, BVH, PAIRS):
        got, st = mctx.intersect(mrays, None, method=method, with_stats=True)
        assert st.method_ran == SCAN and got.tobytes() == mwant.tobytes()
    mctx.close()
    # pageable host hits with device rays, and the other way round
    want = ctx.intersect(rays, None, method=SCAN)
    d_rays, d_hits = DevBuf(rays.nbytes).write(rays), DevBuf(want.nbytes)
    for method in (SCAN, BVH, PAIRS):
        host = np.zeros(len(rays), _lib.HIT_DTYPE)
        ctx.intersect_into(d_rays.ptr, len(rays), host.ctypes.data, method)
        assert host.tobytes() == want.tobytes()
        ctx.intersect_into(rays.ctypes.data, len(rays), d_hits.ptr, method)
        assert d_hits.read().tobytes() == want.tobytes()
    with pytest.raises(_lib.HrtError) as e:  # a device pointer off the records' 16-byte alignment
        ctx.intersect_into(d_rays.ptr + 4, 4, d_hits.ptr, SCAN)
    assert e.value.status == 1
    d_rays.free()
    d_hits.free()
    ctx.close()
