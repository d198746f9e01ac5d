"""Shading in two phases: the kernels built on trace_fused_split play a hit's roulette at
the hit (shade_hit) and compute the surviving lanes' new directions once per bounce batch (shade_dir).
Every case compares frames, segments and triangle tests with the CPU oracle, byte for byte, after
asserting that the arm it is about was exercised."""
import functools

import numpy as np
import pytest

from helpers import SceneCase, _lib, mismatch_report

pytestmark = pytest.mark.gpu

FUSED_SPLIT = [4, 5, 6, 7, 8, 9, 10]  # BUNDLE .. BUNDLE_WQ_L2
SCENES = {"box": (64, 64), "spheres": (64, 48), "cave": (96, 54), "island": (96, 54)}


@functools.lru_cache(maxsize=None)
def _ref(scene, size, spp, bounces, off=1):
    """The oracle's (frame, segments, triangle tests), computed once per shape and never written to."""
    img, _, seg, tt = SceneCase(scene, size, spp, bounces, rng_offset=off).oracle()
    img.setflags(write=False)
    return img, seg, tt


def _trace(ctx, pc):
    ctx.reset_stats()
    ctx.trace(pc)
    st = ctx.stats()
    return ctx.read(_lib.IMG_TRACE), st


def _check(ctx, case, ref, what=""):
    img, st = _trace(ctx, case.push())
    want, seg, tt = ref
    assert np.array_equal(img, want), what + mismatch_report(img, want)
    assert (st.segments, st.tri_tests) == (seg, tt), what
    return st


@pytest.mark.parametrize("variant", FUSED_SPLIT)
@pytest.mark.parametrize("scene", list(SCENES))
def test_material_arms_through_deferred_direction(scene, variant):
    """box: specular probability 0.5 with smoothness 0.7 (adjust_dir's general arm), an invisible light
    mesh (the pass-through continue: a waiting lane with nothing pending), a metal sphere (its normal from
    the hit position before the invisible-light offset).  spheres: fuzz 0.1 and an invisible light sphere.  cave: emission, metal with fuzz.  island:
    all Lambertian (the fast arm).  4 spp, 8 bounces; LITERAL (shade_step as written) gives the same bytes."""
    size = SCENES[scene]
    case = SceneCase(scene, size, 4, 8)
    ref = _ref(scene, size, 4, 8)
    assert ref[1] > size[0] * size[1] * 4  # bounces happened
    # (BUNDLE_BVH_LDS holds island's hierarchy in LDS with leaves of 4, not the auto 2)
    ctx = case.context(variant=variant, options={_lib.OPT_BVH_LEAF_SIZE: 4 if variant == 8 and scene == "island" else 0})
    for k in range(2):  # unplanned, then planned
        _check(ctx, case, ref, f"trace {k}: ")
    ctx.close()
    lit, lseg, ltt = case.gpu(variant=1)
    assert np.array_equal(lit, ref[0]) and (lseg, ltt) == ref[1:]


@pytest.mark.parametrize("variant", [4, 9])
@pytest.mark.parametrize("spp", [1, 2, 3])
@pytest.mark.parametrize("bounces", [0, 1, 2])
def test_bounce_limit_and_short_sample_counts(bounces, spp, variant):
    """A hit on the path's last allowed segment owes no direction: at max_bounces 0 every path is one
    segment and phase B computes nothing; at 1 and 2 the limit ends paths that survived the roulette."""
    case = SceneCase("box", (64, 64), spp, bounces)
    ref = _ref("box", (64, 64), spp, bounces)
    if bounces == 0:
        assert ref[1] == 64 * 64 * spp
    else:
        assert ref[1] > 64 * 64 * spp
    ctx = case.context(variant=variant, options={_lib.OPT_COUNTERS: 2})
    _check(ctx, case, ref)
    d = ctx.diagnostics()
    ctx.close()
    if bounces == 0:
        assert d["bounce_lanes"] == 0 and d["dir_lanes"] == 0
    else:
        assert 0 < d["dir_lanes"] <= d["bounce_lanes"]


@pytest.mark.parametrize("variant", [5, 7, 9])
@pytest.mark.parametrize("sec_batch", [1, 64])
def test_batches_of_every_size(sec_batch, variant):
    """HRT_OPT_SECONDARY_BATCH 1 (a batch as soon as one lane waits: directions computed a lane or two at
    a time) and 64 (only when no primary segment is left), on a ragged 37 x 23 island whose edge tiles
    have inactive lanes."""
    case = SceneCase("island", (37, 23), 4, 8)
    ref = _ref("island", (37, 23), 4, 8)
    assert ref[1] > 37 * 23 * 4
    ctx = case.context(variant=variant, options={_lib.OPT_SECONDARY_BATCH: sec_batch, _lib.OPT_COUNTERS: 2})
    _check(ctx, case, ref)
    d = ctx.diagnostics()
    ctx.close()
    assert d["bounce_iters"] > 0 and d["dir_lanes"] == d["bounce_lanes"]


@pytest.mark.parametrize("variant", [7, 9])
@pytest.mark.parametrize("split", [2, 8, 64])
@pytest.mark.parametrize("scene,size", [("island", (37, 23)), ("box", (45, 33))])
def test_split_items_with_few_active_lanes(scene, size, split, variant):
    """Heavy tiles split into row groups (HRT_OPT_SPLIT with factor 0: every tile heavy): items run with
    8 / split rows active and the other lanes idle from the start, never shading."""
    case = SceneCase(scene, size, 4, 8)
    ref = _ref(scene, size, 4, 8)
    assert ref[1] > size[0] * size[1] * 4
    ctx = case.context(variant=variant, options={_lib.OPT_SPLIT: split, _lib.OPT_SPLIT_FACTOR: 0})
    for k in range(3):  # unplanned, planned from an unsplit trace, planned from a split one
        _check(ctx, case, ref, f"trace {k}: ")
    ctx.close()


def test_frame_runs_and_pixel_pool():
    """hrt_compute_n of 3 frames on a 64 x 64 island with BUNDLE_WQ: one launch whose items run a tile's
    frames as one pixel pool.  Each frame's own hrt_trace equals the oracle's frame; the launch's
    accumulator, last trace image and counters equal the per-frame loop's."""
    size, spp, first, n = (64, 64), 4, 5, 3
    case = SceneCase("island", size, spp, 8)
    loop = case.context(variant=9)
    seg = tt = 0
    for k in range(first, first + n):
        want, s, t = _ref("island", size, spp, 8, k)
        assert s > size[0] * size[1] * spp
        img, _ = _trace(loop, case.push(k))
        assert np.array_equal(img, want), f"frame {k}: " + mismatch_report(img, want)
        loop.accumulate(k)
        seg, tt = seg + s, tt + t
    want_acc, want_trace = loop.read(_lib.IMG_ACCUM), loop.read(_lib.IMG_TRACE)
    loop.close()
    ctx = case.context(variant=9)
    ctx.compute_n(case.push(first), n)
    st = ctx.stats()
    got_acc, got_trace = ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_TRACE)
    ctx.close()
    assert st.last_frames == 3 and st.last_kernel == 9
    assert np.array_equal(got_trace, want_trace), mismatch_report(got_trace, want_trace)
    assert np.array_equal(got_acc, want_acc), mismatch_report(got_acc, want_acc)
    assert (st.segments, st.tri_tests) == (seg, tt)


@pytest.mark.parametrize("variant", FUSED_SPLIT)
def test_counter_invariant_island(variant):
    """No spheres, no invisible mesh: every lane of a bounce batch survived a triangle hit, so phase B
    computed a direction for each (dir_lanes == bounce_lanes), whatever the kernel."""
    case = SceneCase("island", (96, 54), 4, 8)
    ref = _ref("island", (96, 54), 4, 8)
    ctx = case.context(variant=variant, options={_lib.OPT_COUNTERS: 2,
                                                 _lib.OPT_BVH_LEAF_SIZE: 4 if variant == 8 else 0})
    _check(ctx, case, ref)
    d = ctx.diagnostics()
    ctx.close()
    assert d["bounce_lanes"] == ref[1] - 96 * 54 * 4  # every segment after a path's first ran in a batch
    assert d["dir_lanes"] == d["bounce_lanes"]


@pytest.mark.parametrize("variant", [4, 7, 9])
def test_counter_invariant_box(variant):
    """box: a lane enters a batch without a pending direction exactly after passing through the invisible
    light mesh (the pass-through continue); sphere and wall hits all owe one.  The oracle reports a
    frame's segments, not which of them followed a pass-through, so the test cannot count them from it:
    it asserts that the scene has some (dir_lanes < bounce_lanes) and that phase B ran."""
    case = SceneCase("box", (64, 64), 4, 8)
    ref = _ref("box", (64, 64), 4, 8)
    ctx = case.context(variant=variant, options={_lib.OPT_COUNTERS: 2})
    _check(ctx, case, ref)
    d = ctx.diagnostics()
    ctx.close()
    assert d["bounce_lanes"] == ref[1] - 64 * 64 * 4
    assert 0 < d["dir_lanes"] < d["bounce_lanes"]
