"""The sky lane (HRT_OPT_SKY_LANE): a planned BUNDLE_WQ launch's sky items on trace_sky beside the main kernel.

Every expected value comes from the CPU oracle alone (frames folded by the oracle's combiner), computed once
per case and shared: images byte for byte, `segments` and `tri_tests` exact -- the segment counter proves that
every item ran exactly once whichever kernel took it.  A context's first launch on a lane has no plan (images
of fewer than 1,024 tiles take no probe), so every script launches more than once: the later launches are
planned and fork to trace_sky.  All images here have fewer tiles than trace_sky has waves, so its cursor meets
the main kernel's at once -- those cases check the protocol's ends and the join.  That trace_sky itself renders
items right (seeds, frame slots, tile records, runs cut by item ends and by the front cursor) is the business of
test_trace_sky_renders_items, at a size where it must take items and says how many it ran."""
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


def make_case(scene, size, spp, bounces, env=True, sky_camera=False):
    case = SceneCase(scene, size, spp, bounces)
    if not env:
        case.settings.use_environment_lighting = False
    if sky_camera:  # far above the island, looking up: every primary segment is a miss
        case.camera = E.Camera([-5.0, 200.0, -20.0], [0.2, 0.5, 1.0])
    return case


def push(case, k, samples=None, init=False):
    pc = case.push(k, init=init)
    if samples is not None:
        pc.num_samples = samples
    return pc


@functools.lru_cache(maxsize=None)
def oracle_frames(key, n, samples=None, row_ranges=None):
    """Frames 1..n of make_case(*key) by the oracle: ((rgba8 image, segments, tri_tests), ...); the counters
    over the global row ranges row_ranges (a row-tile part's) when given, else over the whole frame."""
    case = make_case(*key)
    out = []
    for k in range(1, n + 1):
        pc = push(case, k, samples)
        img, _, seg, tt = pyoracle.trace(pc, case.rays, case.spheres, case.tris, case.meshes)
        if row_ranges is not None:
            seg = tt = 0
            for rows in row_ranges:
                _, _, s, t = pyoracle.trace(pc, case.rays, case.spheres, case.tris, case.meshes, rows=rows)
                seg, tt = seg + s, tt + t
        out.append((img, seg, tt))
    return tuple(out)


def folded(frames, upto):
    """The oracle's accumulator after the clear (frame 0) and frames 1..upto."""
    acc = np.zeros_like(frames[0][0])
    pyoracle.accumulate_rgba8(0, acc, acc.copy())
    for k in range(1, upto + 1):
        pyoracle.accumulate_rgba8(k, acc, frames[k - 1][0])
    return acc


def drive(key, script, sky=1, samples=None, partition=None, debug=False, options=None, variant=WQ):
    """Runs script -- ("n", k): hrt_compute_n of k frames; ("until", k): hrt_compute_until with a rule no frame
    meets, so k frames; ("loop", k): k x (hrt_trace, hrt_accumulate); ("read", 0): the accumulator read and
    checked in mid-script; ("sky", v): HRT_OPT_SKY_LANE = v -- after a clear, and checks the accumulator, the
    last trace image and the counters against the oracle."""
    case = make_case(*key)
    total = sum(n for kind, n in script if kind in ("n", "until", "loop"))
    opts = {_lib.OPT_SKY_LANE: sky}
    opts.update(options or {})
    ctx = case.context(variant=variant, partition=partition, debug=debug, options=opts)
    rows = ctx.global_rows()
    real = rows < ctx.height
    ranges = None
    if partition is not None:
        starts = rows[real][::partition[0]]
        ranges = tuple((int(y), int(min(y + partition[0], ctx.height))) for y in starts)
    frames = oracle_frames(key, total, samples, ranges)

    def expect_accumulator(upto):
        got, want = ctx.read(_lib.IMG_ACCUM)[real], folded(frames, upto)[rows[real]]
        assert np.array_equal(got, want), f"accumulator after frame {upto}: " + mismatch_report(got, want)

    ctx.trace(push(case, 0, init=True))
    ctx.accumulate(0)
    k = 1
    for kind, n in script:
        if kind == "n":
            ctx.compute_n(push(case, k, samples), n)
            k += n
        elif kind == "until":
            done, settled = ctx.compute_until(push(case, k, samples), n, 0, 0, 1)
            assert (done, settled) == (n, False)
            k += n
        elif kind == "loop":
            for _ in range(n):
                ctx.trace(push(case, k, samples))
                ctx.accumulate(k)
                k += 1
        elif kind == "read":
            expect_accumulator(k - 1)
        else:
            ctx.set_option(_lib.OPT_SKY_LANE, n)
    st = ctx.stats()
    expect_accumulator(total)
    got, want = ctx.read(_lib.IMG_TRACE)[real], frames[total - 1][0][rows[real]]
    kernel = st.last_kernel
    ctx.close()
    assert np.array_equal(got, want), "last trace image: " + mismatch_report(got, want)
    assert (st.segments, st.tri_tests) == (sum(f[1] for f in frames), sum(f[2] for f in frames))
    return frames, kernel


@pytest.mark.parametrize("sky", [1, -1])
@pytest.mark.parametrize("size", [(96, 72), (100, 37)])
def test_island_launches_of_1_2_5_then_until(size, sky):
    """Launches of 1, 2 and 5 frames, then hrt_compute_until (4 frames), with the lane on and on auto."""
    _, kernel = drive(("island", size, 4, 3), [("n", 1), ("n", 2), ("n", 5), ("until", 4)], sky=sky)
    assert kernel == WQ


SKY_ONLY = [("n", 2), ("n", 3), ("loop", 2)]


@pytest.mark.parametrize("size", [(96, 72), (100, 37), (8, 8), (5, 3)])
def test_only_sky(size):
    """A camera that sees only sky: every item is a sky item and the main kernel has none of its own; 8x8 and
    5x3 are exactly one tile.  (Every path is one segment: the oracle's count says the camera sees no triangle.)"""
    key = ("island", size, 4, 3, True, True)
    frames, kernel = drive(key, SKY_ONLY)
    assert kernel == WQ
    assert all(f[1] == size[0] * size[1] * 4 for f in frames)


def test_no_sky_item_from_inside_the_cave():
    """cave from inside: no tile's list is empty, trace_sky ends at once."""
    drive(("cave", (96, 72), 2, 3), [("n", 2), ("n", 3), ("loop", 2)])


@pytest.mark.parametrize("scene", ["spheres", "box"])
def test_scenes_with_spheres_have_no_sky_items(scene):
    """The sky rule excludes scenes with spheres: `spheres` (no mesh: not BUNDLE_WQ at all) and `box` (a sphere
    inside a mesh, BUNDLE_WQ forced) keep every item on the main kernel."""
    drive((scene, (64, 48), 2, 4), [("n", 2), ("n", 3), ("loop", 2)])


def test_environment_light_off():
    drive(("island", (96, 72), 4, 3, False), [("n", 2), ("n", 4), ("loop", 2)])


@pytest.mark.parametrize("samples", [0, 1])
def test_num_samples_0_and_1(samples):
    drive(("island", (96, 72), 4, 3), [("n", 2), ("n", 3), ("loop", 2)], samples=samples)


def test_row_tile_part_with_padding_rows():
    """Part 1 of (8, 1, 3) on 80x70: global rows up to 71, so the part's last tile has padding rows, and whole
    tiles of padding count as sky items.  Real rows only."""
    drive(("island", (80, 70), 2, 3), [("n", 2), ("n", 4), ("loop", 2)], partition=(8, 1, 3))


@pytest.mark.parametrize("limit_frames", [1, 3])
def test_frame_stack_fallback_forks_and_joins_repeatedly(limit_frames):
    """HRT_DEBUG_OPT_STACK_LIMIT (debug library): a stack of at most 3 frames (launches of 3, then 2 + 2), or
    none at all (a launch per frame)."""
    size = (64, 48)
    drive(("island", size, 2, 3), [("n", 3), ("n", 4), ("n", 4)], debug=True,
          options={_lib.OPT_FRAMES_PER_LAUNCH: 8, _lib.DEBUG_OPT_STACK_LIMIT: limit_frames * size[0] * size[1] * 4})


def test_per_frame_loop_on_three_lanes_with_a_read_in_the_middle():
    """hrt_trace / hrt_accumulate x 6 over three trace lanes, each with its own side stream: the join precedes
    the fold of every frame and the read after the third."""
    drive(("island", (96, 72), 4, 3), [("loop", 3), ("read", 0), ("loop", 3)], options={_lib.OPT_OVERLAP: 3})


def test_option_toggled_between_launches():
    drive(("island", (96, 72), 4, 3),
          [("n", 2), ("sky", 0), ("n", 2), ("sky", 1), ("n", 3), ("loop", 1), ("sky", -1), ("n", 2), ("loop", 1)])


def sky_units(ctx):
    v = ctypes.c_uint64()
    ctx._check(ctx.lib.hrt_debug_sky_units(ctx.handle, ctypes.byref(v)), "hrt_debug_sky_units")
    return v.value


BIG = (1920, 1080)
# The first launch also pays the side stream's first use (tens of ms: trace_sky arrives after the main kernel has
# ended); 18 and 7 frames are no multiple of trace_sky's claim of 4, so its claims span two items.
BIG_LAUNCHES = (2, 18, 7, 1)
BIG_SPP = 16  # (a launch of 18 frames takes milliseconds: far longer than a kernel's way through a second queue)


def run_big(sky_camera, sky):
    case = make_case("island", BIG, BIG_SPP, 3, True, sky_camera)
    ctx = case.context(variant=WQ, options={_lib.OPT_SKY_LANE: sky})
    k = 1
    for n in BIG_LAUNCHES:
        ctx.compute_n(case.push(k), n)
        k += n
    st = ctx.stats()
    out = (ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_TRACE), (st.segments, st.tri_tests, st.traces, st.accumulates),
           sky_units(ctx), st.last_kernel)
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def big_reference(sky_camera):
    return run_big(sky_camera, 0)


@pytest.mark.parametrize("sky_camera", [False, True])
def test_trace_sky_renders_items(sky_camera):
    """island 1080p (32,400 tiles; too large for the oracle: the reference is a context with the lane off, which
    runs the kernels of the per-frame loop), 16 spp, launches of 2, 18, 7 and 1 frames with the lane on: 583,200
    work units in the second launch against the main kernel's 4,096 waves, so trace_sky takes items -- the
    library counts the units it ran (hrt_debug_sky_units) -- and the front cursor meets the back one in the
    middle of the sky items, where a front claim is cut.  Accumulator, last trace image and counters are
    those of the lane-off context, which runs no unit on trace_sky; with the camera on the sky alone every
    unit is a sky unit."""
    acc, trace, counters, off_units, _ = big_reference(sky_camera)
    assert off_units == 0
    got_acc, got_trace, got_counters, units, kernel = run_big(sky_camera, 1)
    total = (BIG[0] // 8) * (BIG[1] // 8) * sum(BIG_LAUNCHES)
    assert kernel == WQ
    assert 0 < units <= total, units
    print(f"trace_sky ran {units} of {total} units (sky camera: {sky_camera})")
    assert np.array_equal(got_trace, trace), "last trace image: " + mismatch_report(got_trace, trace)
    assert np.array_equal(got_acc, acc), "accumulator: " + mismatch_report(got_acc, acc)
    assert got_counters == counters
    if sky_camera:
        assert counters[0] == BIG[0] * BIG[1] * BIG_SPP * sum(BIG_LAUNCHES)  # one segment per sample: only sky


def test_option_validation():
    case = make_case("box", (16, 16), 1, 1)
    ctx = case.context()
    for bad in (-2, 2):
        with pytest.raises(_lib.HrtError):
            ctx.set_option(_lib.OPT_SKY_LANE, bad)
    ctx.close()
