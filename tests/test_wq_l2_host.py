"""BUNDLE_WQ_L2's host side (CPU): the breadth-first node image (hrt_bvh.h make_wq_nodes_bfs, through
hrt_debug_bvh_wq_nodes_bfs), the LDS plan (hrt_debug_wq_l2_plan) and the additive ABI.

The kernel keeps the slots below L in LDS and reads the others from global memory, so the image must put
the top of the tree first: groups are allocated level by level, a group stays contiguous, and the child
and escape words name the new slots.  Everything else -- the records, the groups, the leaf ranges -- is
the image BUNDLE_WQ stages (hrt_debug_bvh_wq_nodes), which must come out of this change byte for byte."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from helpers import ROOT, SceneCase, _lib

SCENES = ["box", "island", "cave", "island@2"]
_cases = {}


def case_of(scene):
    if scene not in _cases:
        _cases[scene] = SceneCase(scene, (8, 8), 1, 1)
    return _cases[scene]


def image(case, width, leaf, bfs):
    lib = _lib.load()
    fn = lib.hrt_debug_bvh_wq_nodes_bfs if bfs else lib.hrt_debug_bvh_wq_nodes
    img = np.zeros(70000 * 12, np.float32)
    got = fn(case.tris.ctypes.data, len(case.tris), case.meshes.ctypes.data, len(case.meshes), leaf, width,
             img.ctypes.data, img.size)
    assert got > 0
    return img[:got * 12].view(np.uint32).reshape(got, 12).copy()


def walk(w):
    """The tree below slot 0 as nested tuples that do not name slots: per node its record words 0..9, the
    sin^2 half-word, then the leaf word or the tuple of its group's members; and per slot its depth,
    parent and the escape the structure implies (the next member, else the parent's; the root's: n)."""
    n = len(w)
    depth, parent, esc = np.full(n, -1), np.full(n, -1), np.full(n, -1)
    depth[0], esc[0] = 0, n
    groups = []

    def node(k):
        rec = (w[k, :10].tobytes(), int(w[k, 10]) & 0xFFFF)
        info = int(w[k, 11])
        if info >> 27:
            return rec + (info,)
        fc, cnt = info & 0xFFFF, (info >> 16) + 1
        assert fc + cnt <= n
        groups.append((k, fc, cnt))
        members = []
        for j in range(cnt):
            c = fc + j
            assert depth[c] == -1  # every slot is in one group
            depth[c], parent[c] = depth[k] + 1, k
            esc[c] = c + 1 if j + 1 < cnt else esc[k]
        for j in range(cnt):
            members.append(node(fc + j))
        return rec + (tuple(members),)

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(10000)
    try:
        tree = node(0)
    finally:
        sys.setrecursionlimit(old)
    assert (depth >= 0).all()  # every slot is reached from the root
    return tree, depth, parent, esc, groups


@pytest.mark.parametrize("leaf", [1, 2, 3, 4])
@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("scene", SCENES)
def test_bfs_image_is_the_same_tree_level_by_level(scene, width, leaf):
    case = case_of(scene)
    dfs, bfs = image(case, width, leaf, False), image(case, width, leaf, True)
    assert dfs.shape == bfs.shape
    n = len(bfs)
    t_d, _, _, esc_d, groups_d = walk(dfs)
    t_b, depth, parent, esc_b, groups_b = walk(bfs)
    # the same tree: records (words 0..9 and the sin^2 half-word), leaf ranges, group sizes and member order
    assert t_d == t_b
    assert sorted(c for _, _, c in groups_d) == sorted(c for _, _, c in groups_b)
    # escape = the next member, or the parent's escape; n ends the walk (in both images)
    np.testing.assert_array_equal(dfs[:, 10] >> 16, esc_d)
    np.testing.assert_array_equal(bfs[:, 10] >> 16, esc_b)
    # structure: groups contiguous (walk asserts fc .. fc + cnt - 1 and single membership), parents before
    # children, depth non-decreasing in slot order: "slot < L" is "near the root" for every L
    assert (parent[1:] < np.arange(1, n)).all()
    assert (np.diff(depth) >= 0).all()
    # groups are allocated in the order of their parents' slots
    fcs = [fc for _, fc, _ in sorted(groups_b)]
    assert fcs == sorted(fcs)
    # a stackless walk over the escapes visits every node once
    seen, cur = 0, 0
    while cur != n:
        seen += 1
        assert seen <= n
        info = int(bfs[cur, 11])
        cur = (info & 0xFFFF) if not (info >> 27) else int(bfs[cur, 10] >> 16)
    assert seen == n


# The image BUNDLE_WQ stages as the commit before the breadth-first image built it (width 4, leaves of 4):
# its node count and the SHA-256 of its bytes
DFS_IMAGES = {
    "box": (14, "1ff0f4947e592ac4784cc5cc0257cd8bb3cec1fb9d0776ef5082cdc8272887c8"),
    "island": (781, "0cd3c2ed59a862535feb828c2a804c574b78a5e28867594a6c42d5b5744c80bc"),
    "cave": (1261, "16e1d3c4e240dd6fac3bf2454c44effbed818ddc7f74faa0fd0a82e0422fd68e"),
    "island@2": (3060, "a7614c83db8ca4ad330218974f334002eb31c2325a6303ea96f64f9c073387f9"),
}


@pytest.mark.parametrize("scene", SCENES)
def test_existing_inspector_is_unchanged(scene):
    """hrt_debug_bvh_wq_nodes gives the bytes it gave before this image existed, whether or not the
    breadth-first inspector ran before it; an inner root's group is the first allocated in both images."""
    case = case_of(scene)
    b = image(case, 4, 4, True)
    a = image(case, 4, 4, False)
    assert (len(a), hashlib.sha256(a.tobytes()).hexdigest()) == DFS_IMAGES[scene]
    info = int(a[0, 11])
    if not info >> 27:
        cnt = (info >> 16) + 1
        assert int(b[0, 11]) == info == (1 | (cnt - 1) << 16)
        np.testing.assert_array_equal(a[1:1 + cnt, :10], b[1:1 + cnt, :10])


@pytest.mark.parametrize("opt", [-1, 0, 1, 2, 10**6])
@pytest.mark.parametrize("max_leaf", [1, 2, 3, 4])
@pytest.mark.parametrize("n_nodes", [1, 2, 1109, 1110, 65535])
def test_lds_plan(n_nodes, max_leaf, opt):
    lib = _lib.load()
    out = (ctypes.c_uint32 * 4)()
    lib.hrt_debug_wq_l2_plan(n_nodes, 4, max_leaf, opt, out)
    L, ncap, tcap, nbytes = list(out)
    assert nbytes <= 160 * 1024
    if nbytes == 0:  # "no fit": all four are zero
        assert (L, ncap, tcap) == (0, 0, 0)
    else:
        assert ncap % 64 == 0 and ncap >= 128
        assert tcap == 64 * (1 + 2 * max_leaf)
        assert nbytes == L * 48 + 16 * (512 + 4 * (ncap + tcap))
    assert L <= n_nodes
    # leaves of at most 4 with groups of up to 4: the stacks alone always fit
    assert nbytes > 0
    if opt == 0:
        assert L == 0 and ncap == 1024
    elif opt > 0:
        assert L <= opt
        if opt <= 2:
            assert L == min(opt, n_nodes) and ncap == 1024
    else:  # auto: the stacks at their maximum first, then as many nodes as fit
        assert ncap == 1024
        assert L == n_nodes or nbytes + 48 > 160 * 1024 - 64


def test_lds_plan_rejects_shapes_the_kernel_does_not_take():
    lib = _lib.load()
    out = (ctypes.c_uint32 * 4)()
    for n_nodes, width, max_leaf in [(0, 4, 4), (65536, 4, 4), (100, 1, 4), (100, 5, 4), (100, 4, 5), (100, 4, 16)]:
        lib.hrt_debug_wq_l2_plan(n_nodes, width, max_leaf, -1, out)
        assert list(out) == [0, 0, 0, 0], (n_nodes, width, max_leaf)


def test_abi_is_additive():
    hdr = open(os.path.join(ROOT, "include", "hip_raytrace.h")).read()
    assert re.search(r"#define HRT_ABI_VERSION 6u\b", hdr)
    assert re.search(r"\bHRT_KERNEL_BUNDLE_WQ_L2 = 10\b", hdr)
    assert re.search(r"\bHRT_OPT_WQ_LDS_NODES = 21\b", hdr)
    assert re.search(r"\bHRT_KERNEL_BUNDLE_WQ = 9\b", hdr) and re.search(r"\bHRT_OPT_SKY_LANE = 20\b", hdr)
    assert _lib.KERNEL_BUNDLE_WQ_L2 == 10 and _lib.OPT_WQ_LDS_NODES == 21 and _lib.ABI_VERSION == 6
    assert _lib.KERNEL_NAMES[10] == "bundle_wq_l2"
    assert _lib.load().hrt_abi_version() == 6
