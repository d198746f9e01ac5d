"""The pair traversal after its instruction diet (one selected-address pop per step, stack
offsets counted from the stack's top, the leaf scan skipped in steps that kept no leaf, the leaf entries'
two-level slot select).  What those can break: the push order decides which pairs a step pops, the pops
decide which ray a lane serves, and a skipped scan must leave both stacks as the scan of zeros would --
so every frame below is compared byte for byte, with the exact segment and triangle-test counts, against
the CPU oracle (oracle/pyoracle.py) or against the per-frame loop, and the helpers themselves against a
host model through the debug library's scripted wave (hrt_debug_wq_protocol)."""
import functools

import numpy as np
import pytest

from helpers import SceneCase, mismatch_report
from epq_raytracer_amd import _lib

pytestmark = pytest.mark.gpu

WQ = _lib.KERNEL_BUNDLE_WQ

# scene -> (size, spp); 8 bounces each (box: invisible lights and spheres)
FRAMES = {"box": ((64, 64), 4), "island": ((96, 72), 8), "cave": ((64, 48), 4)}


@functools.lru_cache(maxsize=None)
def _frame(scene):
    """The case and its oracle frame, computed once and shared (never modified)."""
    if scene == "ties":
        from test_gpu_parity import _tie_soup  # coincident triangles within and across meshes
        base = _tie_soup()
        case = SceneCase(settings=base.settings, camera=base.camera, size=(32, 32), num_samples=4, max_bounces=8)
    else:
        size, spp = FRAMES[scene]
        case = SceneCase(scene, size, spp, 8)
    ref, _, seg, tt = case.oracle()
    ref.setflags(write=False)
    return case, ref, seg, tt


def _check_traces(case, ref, seg, tt, variant, options, traces, pinned):
    ctx = case.context(variant=variant, options=options)
    for _ in range(traces):  # (the first trace probes the tiles' costs, the later ones run the plan)
        ctx.reset_stats()
        ctx.trace(case.push())
        st = ctx.stats()
        img = ctx.read(_lib.IMG_TRACE)
        assert np.array_equal(img, ref), mismatch_report(img, ref)
        assert (st.segments, st.tri_tests) == (seg, tt)
        if pinned and ctx.scene_info()["bvh_built"]:
            assert st.last_kernel == WQ
    ctx.close()


CONFIGS = {
    "auto": (0, {}),
    "wq": (WQ, {}),
    "wq_cap128": (WQ, {_lib.OPT_WQ_NODE_CAP: 128}),  # the stackless overflow path on most node steps
    "wq_split1": (WQ, {_lib.OPT_SPLIT: 1}),
    "wq_split8": (WQ, {_lib.OPT_SPLIT: 8, _lib.OPT_SPLIT_FACTOR: 0}),  # every tile split in 8 row groups
}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("scene", list(FRAMES))
def test_trace_bit_exact_against_oracle(scene, config):
    case, ref, seg, tt = _frame(scene)
    variant, options = CONFIGS[config]
    _check_traces(case, ref, seg, tt, variant, options, traces=3 if "split" in config else 2, pinned=variant == WQ)


@pytest.mark.parametrize("config", ["auto", "wq", "wq_cap128"])
def test_tie_soup_bit_exact(config):
    """Coincident triangles (the same soup twice in one mesh and again as a second mesh): equal distances
    whose winner is the scan order, i.e. the closest-hit key -- a changed push order or key shows here."""
    case, ref, seg, tt = _frame("ties")
    variant, options = CONFIGS[config]
    _check_traces(case, ref, seg, tt, variant, options, traces=2, pinned=variant == WQ)


@pytest.mark.parametrize("size,spp", [((96, 72), 3), ((96, 72), 0), ((37, 23), 3)])
def test_multi_frame_launch_matches_frame_loop(size, spp):
    """hrt_compute_n over 5 frames of island with frame runs forced (HRT_DEBUG_OPT_GRAB_RUNS: 4 items per
    grab, so the pixel pool runs, and 1) against five hrt_trace + hrt_accumulate: the accumulator, the
    last trace image and the counters.  spp 0: every pixel-frame ends at once and is still stored; 37x23:
    ragged edge tiles, whose waves run their frames without the pool beside whole tiles that use it."""
    case = SceneCase("island", size, spp, 8)

    def push(k):
        pc = case.push(k)
        pc.num_samples = spp  # (SceneCase clamps to >= 1)
        return pc

    first, n = 3, 5
    loop = case.context(variant=WQ)
    per_frame = []
    for k in range(first, first + n):
        loop.reset_stats()
        loop.trace(push(k))
        loop.accumulate(k)
        st = loop.stats()
        per_frame.append((st.segments, st.tri_tests))
    want_acc, want_trace = loop.read(_lib.IMG_ACCUM), loop.read(_lib.IMG_TRACE)
    loop.close()
    for grab in (1, 0):
        ctx = case.context(variant=WQ, debug=True,
                           options={_lib.OPT_FRAMES_PER_LAUNCH: 16, _lib.DEBUG_OPT_GRAB_RUNS: grab})
        ctx.reset_stats()
        ctx.compute_n(push(first), n)
        b = ctx.stats()
        got_acc, got_trace = ctx.read(_lib.IMG_ACCUM), ctx.read(_lib.IMG_TRACE)
        ctx.close()
        assert b.last_frames == n and b.last_kernel == WQ  # one persistent launch of all n frames
        assert np.array_equal(got_trace, want_trace), f"grab {grab}: " + mismatch_report(got_trace, want_trace)
        assert np.array_equal(got_acc, want_acc), f"grab {grab}: " + mismatch_report(got_acc, want_acc)
        assert (b.segments, b.tri_tests) == tuple(map(sum, zip(*per_frame))), f"grab {grab}"


def _protocol_model(cnt, take):
    """Host model of hrt_debug_wq_protocol's stack with mixed pops (take = nn | tn << 8): the top nn
    entries to lanes [0, nn), the tn below them to lanes [nn, nn + tn), 0xFFFFFFFF elsewhere; then the
    lanes' pushes slot-major in lane order at the stack's top."""
    rounds = len(take)
    stack = []
    popped = np.full((rounds, 64), 0xFFFFFFFF, np.uint64)
    for r in range(rounds):
        nn = min(int(take[r]) & 0xFF, len(stack), 64)
        tn = min(int(take[r]) >> 8, len(stack) - nn, 64 - nn)
        n = len(stack) - nn - tn
        popped[r, :nn] = stack[n + tn:]
        popped[r, nn:nn + tn] = stack[n:n + tn]
        del stack[n:]
        for k in range(4):
            room = len(stack) + 256 <= 8192  # wave-uniform, before the k-th pushes
            for lane in range(64):
                if cnt[r, lane] > k and room:
                    stack.append((r << 16) | (lane << 8) | k)
    return popped, len(stack)


@pytest.mark.parametrize("case", ["mixed", "node_only", "tri_only", "short", "deep"])
def test_pop_and_push_helpers_match_host(case):
    """wq_pop (one load at a selected address: node lanes, triangle lanes, idle lanes) and wq_push's
    offsets counted from the stack's top (lanes_below_from), on 96 scripted rounds of one wave = 6144 lane
    cases per shape: every popped word and the final depth equal the host model's."""
    rng = np.random.default_rng(700 + ["mixed", "node_only", "tri_only", "short", "deep"].index(case))
    rounds = 96
    cnt = rng.integers(0, 5, (rounds, 64)).astype(np.uint32)
    nn = rng.integers(0, 65, rounds)
    tn = rng.integers(0, 65, rounds)
    if case == "node_only":
        tn[:] = 0
    elif case == "tri_only":
        nn[:] = 0
    elif case == "short":  # few pairs of each kind: most lanes idle
        nn, tn = rng.integers(0, 9, rounds), rng.integers(0, 9, rounds)
        cnt[rng.random((rounds, 64)) < 0.8] = 0
    elif case == "deep":   # pushes outrun the pops: offsets from a top far above 2^8
        nn, tn = rng.integers(0, 20, rounds), rng.integers(0, 20, rounds)
    take = (nn | (tn << 8)).astype(np.uint32)
    tgt = np.full((rounds, 64), 64, np.uint32)  # no slot access
    val = np.zeros((rounds, 64), np.uint64)
    seed = np.full(64, 1 << 62, np.uint64)
    popped = np.zeros((rounds, 64), np.uint32)
    seen = np.zeros((rounds, 64), np.uint64)
    slots = np.zeros(64, np.uint64)
    depth = np.zeros(1, np.uint32)
    lib = _lib.load()
    _lib.check(lib.hrt_debug_wq_protocol(0, rounds, _lib.ptr(cnt), _lib.ptr(take), _lib.ptr(tgt), _lib.ptr(val),
                                         _lib.ptr(seed), _lib.ptr(popped), _lib.ptr(seen), _lib.ptr(slots),
                                         _lib.ptr(depth)), "hrt_debug_wq_protocol")
    want_pop, want_depth = _protocol_model(cnt, take)
    assert int(depth[0]) == want_depth
    bad = np.argwhere(popped.astype(np.uint64) != want_pop)
    assert bad.size == 0, f"{len(bad)} popped entries differ, first (round, lane) {bad[:3].tolist()}"
    assert np.array_equal(slots, seed)
