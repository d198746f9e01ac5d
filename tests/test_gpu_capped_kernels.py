"""The register-capped BUNDLE_WQ kernels (trace_bundle_wq<false> / trace_bundle_wq_nr<false>, the ones that run
beside trace_sky) on the paths whose code their register diet moved: the per-wave stack bases, the owner's slot
address, the band rounds' marks and the tile list's length and AABB word.

HRT_OPT_SKY_LANE = 1 is forced, so every planned launch runs the capped kernel.  A trace lane's first launch has no
plan and runs the uncapped one: every trace goes to lane 0 (HRT_OPT_OVERLAP = 1), so only a script's first launch
is unplanned and every script ends with launches of the shapes it checks (the per-frame loop on its three lanes
would run each lane's first frame uncapped).  Every expected value is the CPU oracle's (frames folded by the
oracle's combiner), computed once per scene and shared between the cases: accumulator and last trace image byte
for byte, `segments` and `tri_tests` equal.

That the capped kernels are the ones launched is asserted where it can be: launch_trace starts trace_sky's work and
the capped instantiation under the same flag, so units counted by hrt_debug_sky_units prove both.  The small images
have fewer work units than the main kernel has waves, so there trace_sky may find the plan taken and run nothing
(its count is printed, not asserted); test_lane_takes_items_beside_each_capped_kernel runs each capped kernel at
1080p, where trace_sky must take items, and asserts the count."""
import ctypes
import functools

import numpy as np
import pytest

import epq_raytracer_amd as E
import pyoracle
from epq_raytracer_amd import _lib
from helpers import SceneCase, mismatch_report

pytestmark = pytest.mark.gpu

WQ = 9  # HRT_KERNEL_BUNDLE_WQ
SPP, BOUNCES = 8, 2
WIDE = 500.0


def quad(y, up):
    """Two triangles spanning [-WIDE, WIDE]^2 at height y, facing up or down."""
    a, b, c, d = [-WIDE, y, -WIDE], [WIDE, y, -WIDE], [WIDE, y, WIDE], [-WIDE, y, WIDE]
    return [a, c, b, a, d, c] if up else [a, b, c, a, c, d]


def built_case(heights, size, position, direction):
    """A floor at y = 0 facing up and a ceiling facing down at each of `heights`, one Lambertian mesh."""
    pos = np.asarray(quad(0.0, True) + [v for h in heights for v in quad(h, False)], np.float32)
    camera = E.Camera(position, direction)
    mesh = E.RayTracingMesh(E.Mesh(pos, np.arange(len(pos), dtype=np.uint32)), E.LambertianMaterial([0.7, 0.5, 0.3]))
    settings = E.RayTracerSettings(num_samples=SPP, max_bounces=BOUNCES, use_environment_lighting=True,
                                   mesh_data=[mesh], up=camera.up)
    return SceneCase(None, size, SPP, BOUNCES, settings=settings, camera=camera)


@functools.lru_cache(maxsize=None)
def make_case(name):
    if name == "island":
        return SceneCase("island", (192, 108), SPP, BOUNCES)
    if name == "cave":
        return SceneCase("cave", (96, 54), SPP, BOUNCES)
    if name == "runs":
        return SceneCase("island", (75, 41), 3, BOUNCES)
    if name == "leafroot":  # the floor alone, seen at a slant: the horizon crosses the image (sky tiles above it)
        return built_case([], (64, 64), [0.0, 1.0, 0.0], [1.0, -0.2, 0.3])
    assert name == "burst"  # between the floor and the lowest of three ceilings, looking down: every pixel the floor
    return built_case([1.0, 2.0, 3.0], (32, 32), [0.0, 0.5, 0.0], [0.3, -1.0, 0.2])


def wq_words(case, leaf, width):
    """The BUNDLE_WQ node image's last four words per node, as the library builds it on the host."""
    img = np.zeros(4096 * 12, np.float32)
    got = _lib.load().hrt_debug_bvh_wq_nodes(case.tris.ctypes.data, len(case.tris), case.meshes.ctypes.data,
                                             len(case.meshes), leaf, width, img.ctypes.data, img.size)
    assert got > 0
    return img[:got * 12].reshape(got, 12)[:, 8:12].copy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def oracle_frames(name, n, row_ranges=None):
    """Frames 1..n by the oracle: ((rgba8 image, segments, tri_tests), ...), the counters over the global row ranges
    row_ranges (a row-tile part's) when given."""
    case = make_case(name)
    out = []
    for k in range(1, n + 1):
        pc = case.push(k)
        img, _, seg, tt = pyoracle.trace(pc, case.rays, case.spheres, case.tris, case.meshes)
        if row_ranges is not None:
            seg = tt = 0
            for rows in row_ranges:
                _, _, s, t = pyoracle.trace(pc, case.rays, case.spheres, case.tris, case.meshes, rows=rows)
                seg, tt = seg + s, tt + t
        out.append((img, seg, tt))
    return tuple(out)


def sky_units(ctx):
    v = ctypes.c_uint64()
    ctx._check(ctx.lib.hrt_debug_sky_units(ctx.handle, ctypes.byref(v)), "hrt_debug_sky_units")
    return v.value


N_LOOP_N = (("n", 3), ("loop", 3), ("n", 3))


def drive(name, script=N_LOOP_N, options=None, partition=None, debug=False):
    """After a clear, script's launches -- ("n", k): one hrt_compute_n of k frames; ("loop", k): k x (hrt_trace,
    hrt_accumulate) -- over consecutive frames; then the accumulator, the last trace image and the counters
    against the oracle."""
    case = make_case(name)
    total = sum(n for _, n in script)
    opts = {_lib.OPT_SKY_LANE: 1, _lib.OPT_OVERLAP: 1}
    opts.update(options or {})
    ctx = case.context(variant=WQ, partition=partition, debug=debug, options=opts)
    rows = ctx.global_rows()
    real = rows < ctx.height
    ranges = None
    if partition is not None:
        starts = rows[real][::partition[0]]
        ranges = tuple((int(y), int(min(y + partition[0], ctx.height))) for y in starts)
    frames = oracle_frames(name, total, ranges)
    want_acc = np.zeros_like(frames[0][0])
    pyoracle.accumulate_rgba8(0, want_acc, want_acc.copy())
    for k in range(1, total + 1):
        pyoracle.accumulate_rgba8(k, want_acc, frames[k - 1][0])
    ctx.trace(case.push(0, init=True))
    ctx.accumulate(0)
    ctx.reset_stats()
    k = 1
    for kind, n in script:
        if kind == "n":
            ctx.compute_n(case.push(k), n)
            k += n
        else:
            for _ in range(n):
                ctx.trace(case.push(k))
                ctx.accumulate(k)
                k += 1
    st = ctx.stats()
    got_acc, got = ctx.read(_lib.IMG_ACCUM)[real], ctx.read(_lib.IMG_TRACE)[real]
    print(f"{name}: trace_sky ran {sky_units(ctx)} units")
    ctx.close()
    assert st.last_kernel == WQ
    want = frames[total - 1][0][rows[real]]
    assert np.array_equal(got, want), "last trace image: " + mismatch_report(got, want)
    assert np.array_equal(got_acc, want_acc[rows[real]]), "accumulator: " + mismatch_report(got_acc, want_acc[rows[real]])
    assert (st.segments, st.tri_tests) == (sum(f[1] for f in frames), sum(f[2] for f in frames))


PATHS = {"base": {},
         "node_cap_128": {_lib.OPT_WQ_NODE_CAP: 128},     # the node stack overflows: the stackless walk
         "node_radius": {_lib.OPT_WQ_NODE_RADIUS: 2},     # trace_bundle_wq_nr<false>
         "split_8": {_lib.OPT_SPLIT: 8, _lib.OPT_SPLIT_FACTOR: 0}}  # every tile heavy: row groups, idle lanes


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["island", "cave"])
def test_frames_equal_the_oracle(name, path):
    """island 192x108 and cave 96x54, 8 spp, 2 bounces: 3 frames in one hrt_compute_n, 3 as the per-frame loop and 3
    more in one launch."""
    drive(name, options=PATHS[path])


def test_leaf_root_pushes_its_triangles():
    """A scene of two triangles: the hierarchy's root is a leaf, whose triangles every bounce ray pushes itself
    (the triangle stack's second user)."""
    case = make_case("leafroot")
    w = wq_words(case, 2, 4)
    assert len(w) == 1 and w[0, 3] >> 27 == 2
    drive("leafroot", options={_lib.OPT_BVH_LEAF_SIZE: 2, _lib.OPT_BVH_WIDTH: 4})


@pytest.mark.parametrize("tri_cap", [0, 128])
def test_leaf_burst_beyond_the_triangle_stack(tri_cap):
    """A root group of four leaves of two (checked on the host's hierarchy): the floor and three wide ceilings facing
    it.  Every pixel's first bounce leaves the floor upwards and crosses all three ceilings' boxes, which one node
    step tests together: 6 kept triangles per ray, 384 for a tile's 64 rays in one step, against a triangle stack of
    64 x (1 + 2 x 2) = 320 entries -- the step's lanes test their leaves in place.  That the batch holds the 54 rays
    it takes is argued, not observed, so the case runs again with the debug library's HRT_DEBUG_OPT_WQ_TRI_CAP = 128,
    where 22 rays are enough and a step of one tile's rays overflows for certain."""
    case = make_case("burst")
    w = wq_words(case, 2, 4)
    root = int(w[0, 3])
    assert root >> 27 == 0 and root >> 16 == 3  # an inner root whose group has four members
    fc = root & 0xFFFF
    assert len(w) == 5 and all(int(w[fc + j, 3]) >> 27 == 2 for j in range(4))
    options = {_lib.OPT_BVH_LEAF_SIZE: 2, _lib.OPT_BVH_WIDTH: 4}
    if tri_cap:
        options[_lib.DEBUG_OPT_WQ_TRI_CAP] = tri_cap
    drive("burst", debug=bool(tri_cap), options=options)


def test_frame_runs_with_the_pixel_pool():
    """island 75x41, 3 spp: the debug library's HRT_DEBUG_OPT_GRAB_RUNS makes a wave take 4 frames of a tile per grab
    at this size, which run as one pass over a pool of pixel-frames (launches of 1, 8 and 4 frames)."""
    drive("runs", script=(("n", 1), ("n", 8), ("n", 4)), debug=True,
          options={_lib.OPT_FRAMES_PER_LAUNCH: 16, _lib.DEBUG_OPT_GRAB_RUNS: 1})


@pytest.mark.parametrize("part", [0, 1])
def test_row_tile_partition_of_two(part):
    """Both parts of a 2-part row-tile partition of island 192x108 (108 rows: the last tile row is ragged)."""
    drive("island", partition=(8, part, 2))


BIG = (1920, 1080)
BIG_LAUNCHES = (2, 18)  # the first has no plan; the second is planned: 583,200 work units against 4,096 waves


def run_big(sky, options):
    case = SceneCase("island", BIG, 16, BOUNCES)
    opts = {_lib.OPT_SKY_LANE: sky}
    opts.update(options)
    ctx = case.context(variant=WQ, options=opts)
    k = 1
    for n in BIG_LAUNCHES:
        ctx.compute_n(case.push(k), n)
        k += n
    st = ctx.stats()
    out = (ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_TRACE), (st.segments, st.tri_tests), sky_units(ctx), st.last_kernel)
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def big_reference():
    """Lane off, default options: the uncapped kernels, whose code is not under test here."""
    return run_big(0, {})


@pytest.mark.parametrize("path", ["base", "node_cap_128", "node_radius"])
def test_lane_takes_items_beside_each_capped_kernel(path):
    """island 1080p, 16 spp (too large for the oracle: the reference is a context with the lane off, as in
    test_trace_sky_renders_items), launches of 2 and 18 frames with the lane on: trace_sky takes items of the second,
    which launch_trace starts only together with the capped kernel -- trace_bundle_wq<false>, the same with the
    stackless walk, and trace_bundle_wq_nr<false>.  Accumulator, last trace image and counters are those of the
    lane-off context (none of the three options changes a result), which runs no unit on trace_sky."""
    acc, trace, counters, off_units, _ = big_reference()
    assert off_units == 0
    got_acc, got_trace, got_counters, units, kernel = run_big(1, PATHS[path])
    total = (BIG[0] // 8) * (BIG[1] // 8) * sum(BIG_LAUNCHES)
    print(f"{path}: trace_sky ran {units} of {total} units")
    assert kernel == WQ
    assert 0 < units <= total, units
    assert np.array_equal(got_trace, trace), "last trace image: " + mismatch_report(got_trace, trace)
    assert np.array_equal(got_acc, acc), "accumulator: " + mismatch_report(got_acc, acc)
    assert got_counters == counters
