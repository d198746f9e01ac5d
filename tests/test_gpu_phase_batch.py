"""The fused loop's two thresholds: HRT_OPT_SECONDARY_BATCH says when a wave runs its waiting
lanes' bounce segments, HRT_OPT_PRIMARY_BATCH from how many ready lanes a trip that runs a batch runs the
primary phase too; a lane held back starts its sample in the trip that runs it.  Only the trip a segment runs
in moves: every case compares frames, segments and triangle tests with the CPU oracle, byte for byte, after
asserting that bounces happened, and the diagnostics kernel's lane counts must not depend on the thresholds."""
import functools
import itertools

import numpy as np
import pytest

from helpers import SceneCase, _lib, mismatch_report

pytestmark = pytest.mark.gpu

FUSED_SPLIT = [4, 5, 6, 7, 8, 9, 10]  # BUNDLE .. BUNDLE_WQ_L2: the kernels built on trace_fused_split
SHAPES = {"box": ("box", (64, 64)), "spheres": ("spheres", (64, 64)), "island": ("island", (64, 64)),
          "cave": ("cave", (64, 64)), "ragged": ("island", (37, 23))}
PRIM, SEC = (1, 8, 32, 64), (1, 28, 64)
WQ = 9


@functools.lru_cache(maxsize=None)
def _ref(scene, size, spp, bounces, off=1, rows=None):
    """The oracle's (frame, segments, triangle tests), computed once per shape and never written to."""
    img, _, seg, tt = SceneCase(scene, size, spp, bounces, rng_offset=off).oracle(rows=rows)
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


def _thresholds(ctx, prim, sec):
    ctx.set_option(_lib.OPT_PRIMARY_BATCH, prim)
    ctx.set_option(_lib.OPT_SECONDARY_BATCH, sec)


@pytest.mark.parametrize("variant", FUSED_SPLIT)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_pair_of_thresholds(shape, variant):
    """4 spp, 8 bounces; the twelve pairs on one context (its first trace unplanned, the others planned)."""
    scene, size = SHAPES[shape]
    case = SceneCase(scene, size, 4, 8)
    ref = _ref(scene, size, 4, 8)
    assert ref[1] > size[0] * size[1] * 4  # bounces happened
    # (BUNDLE_BVH_LDS holds island's hierarchy in LDS with leaves of 4, not the auto 2)
    ctx = case.context(variant=variant, options={_lib.OPT_BVH_LEAF_SIZE: 4 if variant == 8 and scene == "island" else 0})
    for prim, sec in itertools.product(PRIM, SEC):
        _thresholds(ctx, prim, sec)
        _check(ctx, case, ref, f"primary {prim}, secondary {sec}: ")
    ctx.close()


@pytest.mark.parametrize("variant", [4, 9])
@pytest.mark.parametrize("spp", [1, 2, 3])
@pytest.mark.parametrize("bounces", [0, 1, 2])
def test_short_paths_and_sample_counts(bounces, spp, variant):
    """box at max_bounces 0-2 x num_samples 1-3.  At 0 bounces no lane ever waits: no batch runs, nothing is
    deferred and every trip is a primary trip, whatever the thresholds."""
    case = SceneCase("box", (64, 64), spp, bounces)
    ref = _ref("box", (64, 64), spp, bounces)
    if bounces == 0:
        assert ref[1] == 64 * 64 * spp
    else:
        assert ref[1] > 64 * 64 * spp
    ctx = case.context(variant=variant, options={_lib.OPT_COUNTERS: 2})
    for prim, sec in [(1, 1), (32, 28), (64, 64), (48, 1)]:
        _thresholds(ctx, prim, sec)
        _check(ctx, case, ref, f"primary {prim}, secondary {sec}: ")
        d = ctx.diagnostics()  # (of this trace: reset_stats zeroes them with the other counters)
        if bounces == 0:
            assert d["bounce_iters"] == 0 and d["batch_only_iters"] == 0 and d["primary_deferred"] == 0
            assert d["loop_iters"] == d["primary_iters"] - spp * d["sky_items"]
        else:
            assert d["bounce_iters"] > 0
    ctx.close()


def test_frame_runs_and_pixel_pool():
    """hrt_compute_n of 3 frames on a 64 x 64 island with BUNDLE_WQ at a primary threshold of 48: one launch
    whose items run a tile's frames as one pixel pool, a deferred lane taking its pool entry at the loop top
    and starting it later.  Each frame's own hrt_trace equals the oracle's frame; the launch's accumulator,
    last trace image and counters equal the per-frame loop's."""
    size, spp, first, n = (64, 64), 4, 5, 3
    case = SceneCase("island", size, spp, 8)
    loop = case.context(variant=WQ, options={_lib.OPT_PRIMARY_BATCH: 48})
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
    ctx = case.context(variant=WQ, options={_lib.OPT_PRIMARY_BATCH: 48})
    ctx.compute_n(case.push(first), n)
    st = ctx.stats()
    got_acc, got_trace = ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_TRACE)
    ctx.close()
    assert st.last_frames == 3 and st.last_kernel == WQ
    assert np.array_equal(got_trace, want_trace), mismatch_report(got_trace, want_trace)
    assert np.array_equal(got_acc, want_acc), mismatch_report(got_acc, want_acc)
    assert (st.segments, st.tri_tests) == (seg, tt)


@pytest.mark.parametrize("variant", [7, 9])
@pytest.mark.parametrize("scene,size", [("island", (37, 23)), ("box", (45, 33))])
def test_split_items_scale_both_thresholds(scene, size, variant):
    """HRT_OPT_SPLIT = 8 with every tile heavy: planned items are row groups of 8 active lanes, for which a
    primary threshold of 48 means 6 ready lanes and the bounce threshold 4 (28) or 8 (64) waiting ones."""
    case = SceneCase(scene, size, 4, 8)
    ref = _ref(scene, size, 4, 8)
    assert ref[1] > size[0] * size[1] * 4
    ctx = case.context(variant=variant, options={_lib.OPT_SPLIT: 8, _lib.OPT_SPLIT_FACTOR: 0, _lib.OPT_PRIMARY_BATCH: 48})
    for k, sec in enumerate((0, 28, 64)):  # unplanned, planned from an unsplit trace, planned from a split one
        ctx.set_option(_lib.OPT_SECONDARY_BATCH, sec)
        _check(ctx, case, ref, f"trace {k}: ")
    ctx.close()


@pytest.mark.parametrize("part", [0, 1])
def test_row_tile_partition_of_two(part):
    """Each part of a 2-part partition of a 64 x 64 island (row tile 32: part p holds rows 32 p .. 32 p + 31)
    at a primary threshold of 48: its rows, segments and triangle tests against the oracle's for those rows."""
    size = (64, 64)
    case = SceneCase("island", size, 4, 8)
    want, seg, tt = _ref("island", size, 4, 8, 1, (32 * part, 32 * part + 32))
    assert seg > 32 * 64 * 4
    ctx = case.context(variant=WQ, partition=(32, part, 2), options={_lib.OPT_PRIMARY_BATCH: 48})
    rows = ctx.global_rows()
    assert rows.tolist() == list(range(32 * part, 32 * part + 32))
    for k in range(2):  # unplanned, then planned
        img, st = _trace(ctx, case.push())
        assert np.array_equal(img, want[rows]), f"trace {k}: " + mismatch_report(img, want[rows])
        assert (st.segments, st.tri_tests) == (seg, tt), f"trace {k}"
    ctx.close()


@pytest.mark.parametrize("variant", FUSED_SPLIT)
@pytest.mark.parametrize("scene", ["box", "spheres"])
def test_schedule_invariants(scene, variant):
    """The diagnostics kernel on a view without sky items (asserted first: PRIMARY_ITERS then counts fused trips
    only; a scene with spheres has none, and box is closed in as well).  A primary lane is a sample's start and a bounce lane a later segment of its path, so neither sum
    depends on the thresholds; every counted trip ran a phase; and at a primary threshold of 1 nothing is
    deferred: the trips without the primary phase are exactly those with no ready lane."""
    size = (64, 64)
    case = SceneCase(scene, size, 4, 8)
    ref = _ref(scene, size, 4, 8)
    assert ref[1] > size[0] * size[1] * 4
    ctx = case.context(variant=variant, options={_lib.OPT_COUNTERS: 2})
    lanes = set()
    for prim, sec in itertools.product((1, 8, 32, 48, 64), (1, 28, 44, 64)):
        _thresholds(ctx, prim, sec)
        _check(ctx, case, ref, f"primary {prim}, secondary {sec}: ")
        d = ctx.diagnostics()
        what = f"primary {prim}, secondary {sec}: {d}"
        assert d["sky_items"] == 0, what
        lanes.add((d["primary_lanes"], d["bounce_lanes"]))
        assert d["primary_lanes"] == size[0] * size[1] * 4 and d["bounce_lanes"] == ref[1] - d["primary_lanes"], what
        assert max(d["primary_iters"], d["bounce_iters"]) <= d["loop_iters"] <= d["primary_iters"] + d["bounce_iters"], what
        assert d["batch_only_iters"] == d["loop_iters"] - d["primary_iters"], what
        if prim == 1:
            assert d["primary_deferred"] == 0, what
        else:  # (fewer than the threshold's lanes were held back each time)
            assert d["primary_deferred"] <= (prim - 1) * d["batch_only_iters"], what
    assert len(lanes) == 1
    ctx.close()
