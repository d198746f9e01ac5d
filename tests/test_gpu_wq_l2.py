"""HRT_KERNEL_BUNDLE_WQ_L2 (10) on the device: the pair traversal with the node image read from global
memory and the top of the tree (HRT_OPT_WQ_LDS_NODES) in LDS.  Every frame is compared bitwise with the CPU
oracle, segment and triangle-test counters included, and hrt_stats.last_kernel names the kernel that ran.

The shapes are the smallest at which each path can go wrong: the residency boundary L at 0, inside the root's
group (2: a group that straddles LDS and global memory), a few levels down and past the image; a scene
whose image does not fit the LDS at all (island@2, island@4); the stackless walk and the in-place triangle
bursts over global nodes; both node-radius kernels; the diagnostics instantiation; multi-frame launches
and row-tile parts; and the fall-back when the image does not exist."""
import ctypes

import numpy as np
import pytest

from helpers import E, SceneCase, _lib, mismatch_report

pytestmark = pytest.mark.gpu

L2, WQ = _lib.KERNEL_BUNDLE_WQ_L2, _lib.KERNEL_BUNDLE_WQ

_cases, _refs = {}, {}


def case_of(scene, size, spp, bounces):
    key = (scene, size, spp, bounces)
    if key not in _cases:
        _cases[key] = SceneCase(scene, size, spp, bounces)
        _refs[key] = _cases[key].oracle()
    ref, _, seg, tt = _refs[key]
    return _cases[key], ref, seg, tt


def trace_equals(ctx, case, ref, seg, tt, what, kernel=L2):
    ctx.reset_stats()
    ctx.trace(case.push())
    st = ctx.stats()
    img = ctx.read(_lib.IMG_TRACE)
    assert st.last_kernel == kernel, (what, st.last_kernel)
    assert np.array_equal(img, ref), f"{what}: " + mismatch_report(img, ref)
    assert (st.segments, st.tri_tests) == (seg, tt), what
    return img


def root_group_members(case, leaf):
    img = np.zeros(70000 * 12, np.float32)
    n = _lib.load().hrt_debug_bvh_wq_nodes_bfs(case.tris.ctypes.data, len(case.tris), case.meshes.ctypes.data,
                                               len(case.meshes), leaf, 4, img.ctypes.data, img.size)
    assert n > 0
    info = int(img[:12].view(np.uint32)[11])
    return 0 if info >> 27 else (info >> 16) + 1


@pytest.mark.parametrize("scene", ["box", "cube", "island", "cave"])
def test_residency_boundary(scene):
    """L = 0 (every node from global memory), 1 (the root alone in LDS), 2 (the root's group split between
    LDS and global memory), 5, 64 and auto (these images fit whole): the same bytes and counts."""
    case, ref, seg, tt = case_of(scene, (48, 40), 2, 8)
    # whatever leaf size hrt_set_scene picks, the root's group sits at slots 1.. and has >= 2 members:
    # L = 2 keeps its first member in LDS and reads the others from global memory
    for leaf in (1, 2, 3, 4):
        assert root_group_members(case, leaf) >= 2
    ctx = case.context(variant=L2)
    for lds_nodes in (0, 1, 2, 5, 64, -1):
        ctx.set_option(_lib.OPT_WQ_LDS_NODES, lds_nodes)
        trace_equals(ctx, case, ref, seg, tt, f"{scene} L={lds_nodes}")
    ctx.close()


def test_scene_that_does_not_fit_the_lds():
    """island@2: BUNDLE_WQ's image does not fit beside the stacks (it resolves to another kernel);
    BUNDLE_WQ_L2 runs it with the top of the tree in LDS and the rest from global memory."""
    case, ref, seg, tt = case_of("island@2", (96, 64), 2, 8)
    ctx = case.context(variant=WQ)
    ctx.trace(case.push())
    assert ctx.stats().last_kernel != WQ
    ctx.set_option(_lib.OPT_KERNEL_VARIANT, L2)  # (uploads the breadth-first image of the scene already set)
    trace_equals(ctx, case, ref, seg, tt, "island@2 auto L")
    ctx.set_option(_lib.OPT_WQ_LDS_NODES, 0)
    trace_equals(ctx, case, ref, seg, tt, "island@2 L=0")
    ctx.close()


def test_island_at_4():
    """25,472 triangles: against the oracle and against BUNDLE_BVH, which AUTO runs there today."""
    case, ref, seg, tt = case_of("island@4", (64, 48), 1, 4)
    ctx = case.context(variant=L2)
    img = trace_equals(ctx, case, ref, seg, tt, "island@4")
    ctx.set_option(_lib.OPT_KERNEL_VARIANT, _lib.KERNEL_BUNDLE_BVH)
    other = trace_equals(ctx, case, ref, seg, tt, "island@4 BUNDLE_BVH", kernel=_lib.KERNEL_BUNDLE_BVH)
    ctx.close()
    assert np.array_equal(img, other)


FORCED = {
    "node_cap_128": ({_lib.OPT_WQ_NODE_CAP: 128}, False),          # the stackless walk over global nodes
    "tri_cap_128": ({_lib.DEBUG_OPT_WQ_TRI_CAP: 128}, True),       # kept leaves tested in place
    "node_radius_1": ({_lib.OPT_WQ_NODE_RADIUS: 1}, False),
    "node_radius_2": ({_lib.OPT_WQ_NODE_RADIUS: 2}, False),
    "width_2": ({_lib.OPT_BVH_WIDTH: 2}, False),
    "width_3": ({_lib.OPT_BVH_WIDTH: 3}, False),
    "leaf_1": ({_lib.OPT_BVH_LEAF_SIZE: 1}, False),
    "leaf_4": ({_lib.OPT_BVH_LEAF_SIZE: 4}, False),
    "counters_2": ({_lib.OPT_COUNTERS: 2}, False),                 # the diagnostics instantiation
}


@pytest.mark.parametrize("path", sorted(FORCED))
@pytest.mark.parametrize("scene", ["island", "cave"])
def test_forced_paths(scene, path):
    """Each forced path with L = 5, so that both node sources are read."""
    case, ref, seg, tt = case_of(scene, (48, 40), 2, 8)
    options, debug = FORCED[path]
    ctx = case.context(variant=L2, options={_lib.OPT_WQ_LDS_NODES: 5, **options}, debug=debug)
    trace_equals(ctx, case, ref, seg, tt, f"{scene} {path}")
    if path == "counters_2":
        d = ctx.diagnostics()
        assert d["bvh_visits"] > 0 and d["wq_members"] > 0  # the pair traversal's counters were filled
    ctx.close()


def test_compute_n_equals_the_frame_loop():
    case = SceneCase("island@2", (48, 40), 2, 8)
    first, n = 3, 3
    loop = case.context(variant=L2)
    for k in range(first, first + n):
        loop.trace(case.push(k))
        loop.accumulate(k)
    a = loop.stats()
    want_acc, want_trace = loop.read(_lib.IMG_ACCUM), loop.read(_lib.IMG_TRACE)
    loop.close()
    ctx = case.context(variant=L2)
    ctx.compute_n(case.push(first), n)
    b = ctx.stats()
    got_acc, got_trace = ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_TRACE)
    ctx.close()
    assert a.last_kernel == b.last_kernel == L2
    assert b.last_frames == n
    assert np.array_equal(got_trace, want_trace) and np.array_equal(got_acc, want_acc)
    assert (b.segments, b.tri_tests, b.traces, b.accumulates) == (a.segments, a.tri_tests, a.traces, a.accumulates)


def test_row_tile_part_equals_its_rows_of_the_frame():
    from epq_raytracer_amd import rowtiles
    case = SceneCase("island@2", (48, 40), 2, 8)
    whole = case.context(variant=L2)
    whole.trace(case.push())
    full = whole.read(_lib.IMG_TRACE)
    assert whole.stats().last_kernel == L2
    whole.close()
    part = case.context(variant=L2, partition=(8, 1, 2))
    part.trace(case.push())
    got = part.read(_lib.IMG_TRACE)
    assert part.stats().last_kernel == L2
    part.close()
    rows = rowtiles.global_rows(40, 8, 2, 1)
    valid = rows < 40
    assert valid.any()
    assert np.array_equal(got[valid], full[rows[valid]])


def test_fallback_without_a_hierarchy():
    """70 meshes: no hierarchy is built, so no image exists; BUNDLE_WQ_L2 runs what BUNDLE_WQ runs."""
    rng = np.random.default_rng(5)
    meshes = []
    for _ in range(70):
        c = rng.uniform(-4, 4, 3)
        v = (c + rng.uniform(-1, 1, (3, 3))).astype(np.float32)
        meshes.append(E.RayTracingMesh(E.Mesh(v, np.arange(3, dtype=np.uint32)),
                                       E.LambertianMaterial(list(rng.uniform(0.2, 0.9, 3)))))
    st = E.RayTracerSettings(num_samples=2, max_bounces=5, use_environment_lighting=True, mesh_data=meshes)
    case = SceneCase(settings=st, camera=E.Camera([0.0, 0.0, -12.0], [0.0, 0.0, 1.0]), size=(48, 40),
                     num_samples=2, max_bounces=5)
    ref, _, seg, tt = case.oracle()
    ran = {}
    for variant in (WQ, L2):
        ctx = case.context(variant=variant)
        assert ctx.scene_info()["bvh_built"] == 0
        ctx.trace(case.push())
        s = ctx.stats()
        img = ctx.read(_lib.IMG_TRACE)
        ctx.close()
        ran[variant] = s.last_kernel
        assert np.array_equal(img, ref), mismatch_report(img, ref)
        assert (s.segments, s.tri_tests) == (seg, tt)
    assert ran[L2] == ran[WQ] and ran[L2] not in (WQ, L2)


@pytest.mark.parametrize("scene,size,lds_nodes", [("island", (48, 40), 2), ("island@2", (96, 64), -1)])
def test_guard_bands(scene, size, lds_nodes):
    """libhip_raytrace_debug.so: no buffer's guard band is written (the image's upload included)."""
    case, ref, seg, tt = case_of(scene, size, 2, 8)
    ctx = case.context(variant=L2, options={_lib.OPT_WQ_LDS_NODES: lds_nodes}, debug=True)
    trace_equals(ctx, case, ref, seg, tt, f"{scene} debug")
    n, bad = ctx.check_guards()
    ctx.close()
    assert n > 0 and bad == 0


def test_variant_and_option_values():
    case = SceneCase("box", (16, 16), 1, 1)
    ctx = case.context(variant=L2)
    with pytest.raises(_lib.HrtError):
        ctx.set_option(_lib.OPT_KERNEL_VARIANT, 11)
    with pytest.raises(_lib.HrtError):
        ctx.set_option(_lib.OPT_WQ_LDS_NODES, -2)
    ctx.close()
    out = (ctypes.c_uint32 * 4)()
    _lib.load().hrt_debug_wq_l2_plan(3060, 4, 4, -1, out)
    assert out[0] > 0 and out[3] <= 160 * 1024
