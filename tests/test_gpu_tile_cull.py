"""The primary tile lists after the corner-direction rule: build_tile_list's cap rule, then the
four linear forms at the corner directions of the tile's box and of every pixel's jitter box.

Lists come from hrt_debug_tile_lists (refine = 0: the cap rule alone, the lists before this rule; refine = 1: the
product's), the ground truth from tools/tile_cull_model.py: a float64 Moller-Trumbore test of float32 primary
directions formed as get_ray_dir forms them, and the rules themselves in the kernel's float32 arithmetic.

Cases: island 192x108, cave 96x54, box 64x64, a ragged 37x23 island and a built "needle" scene at 64x40 (slivers
whose long edge points along the view ray, acute vertices just inside and outside tile and pixel corners: what the
cap rule was loose on and the corner rule must stay safe on), each from two cameras at 8 spp and 2 bounces.
References are computed once per case and shared."""
import functools
import os
import sys

import numpy as np
import pytest

import epq_raytracer_amd as E
import pyoracle
from epq_raytracer_amd import _lib
from helpers import ROOT, SceneCase, mismatch_report

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tile_cull_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

WQ = 9  # HRT_KERNEL_BUNDLE_WQ
SPP, BOUNCES = 8, 2
SCENES = {"island": ("island", (192, 108)), "cave": ("cave", (96, 54)), "box": ("box", (64, 64)),
          "ragged": ("island", (37, 23)), "needle": (None, (64, 40))}
# Two cameras per scene (None: the preset's).  The VGPR list holds 64 entries; a tile whose survivors do not fit has
# no list (ok = 0) and the soundness test may skip at most 5% of the tiles for that, so island, cave and the ragged
# island are seen from close by, where a tile of these small images holds fewer triangles (checked with the model on
# the CPU: island 0 and 0 of 336 tiles, cave 0 and 1 of 84, ragged 0 and 0 of 15; from the island preset's camera 21 of
# 336 overflow, so that view is an extra case of the list tests only).
CAMERAS = {"island": [([-1.0, 3.0, -6.0], [0.15, -0.4, 1.0]), ([0.0, 2.0, -4.0], [0.0, -0.3, 1.0]), None],
           "cave": [([0.0, 2.0, 0.0], [1.0, -0.3, 0.2]), ([0.0, 2.0, 0.0], [-1.0, -0.5, 0.3])],
           "box": [None, ([1.3, 1.5, 0.4], [-1.0, -0.45, -0.3])],
           "ragged": [([-8.19, 0.82, 8.99], [0.27, -3.61, -0.96]), ([3.58, 6.98, 7.16], [0.66, -2.2, 1.14])],
           "needle": [None, ([0.3, 1.1, -0.2], [0.1, -0.2, 1.0])]}
CASES = [(name, cam) for name in SCENES for cam in (0, 1)]
LIST_CASES = CASES + [("island", 2)]
NEEDLE_CAMERA = ([0.0, 1.0, 0.0], [0.25, -0.1, 1.0])


def needle_settings(camera, size):
    """Slivers placed in the camera's own ray space: a vertex at nc = (1, y, z) and depth s is cam_pos + s M nc.
    Every sliver has its apex at a tile corner of the size's grid (or a pixel corner inside a tile) moved by a small
    multiple of the jitter in or out, its second vertex FAR behind the apex on almost the same ray (the long edge
    points along the view ray: |e x ao| << |e||ao|), and a third vertex off to one side, so the acute screen-space
    vertex sits just inside or just outside the corner."""
    rays, _, jit = E.create_rays(size, 1.0, 2.0, camera.up)
    cen = rays["sample_centre"][:size[0] * size[1], :3].reshape(size[1], size[0], 3).astype(np.float64)
    M = E.view_matrix(camera.direction, camera.up).astype(np.float64).reshape(4, 4).T[:3, :3]  # column-major
    o = np.asarray(camera.position, np.float64)
    rng = np.random.default_rng(0x71E)
    pos = []
    step_y, step_z = cen[1, 0] - cen[0, 0], cen[0, 1] - cen[0, 0]
    for ty in range(1, size[1] // 8):
        for tx in range(1, size[0] // 8):
            for inner in (0, 3):  # the tile corner, and a pixel corner 3 pixels inside the tile
                corner = cen[ty * 8 + inner, tx * 8 + inner] - 0.5 * (step_y + step_z)
                out = rng.choice([-1.0, 1.0], 2)
                apex = corner + np.array([0.0, out[0], out[1]]) * jit * rng.choice([0.02, 0.5, 1.5])
                far = apex + np.array([0.0, out[0], out[1]]) * jit * rng.uniform(0.05, 0.4)
                side = apex + np.array([0.0, out[0] * rng.uniform(0.5, 3.0), -out[1] * rng.uniform(0.0, 0.3)]) * 4 * jit
                s0 = rng.uniform(2.0, 6.0)
                tri = [o + s0 * (M @ apex), o + s0 * rng.uniform(8.0, 40.0) * (M @ far), o + s0 * 1.2 * (M @ side)]
                n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
                if np.dot(o - tri[0], n) <= 0:  # face the camera
                    tri[1], tri[2] = tri[2], tri[1]
                pos += tri
    pos = np.asarray(pos, np.float32)
    half = (len(pos) // 6) * 3
    meshes = [E.RayTracingMesh(E.Mesh(pos[:half], np.arange(half, dtype=np.uint32)), E.LambertianMaterial([0.7, 0.4, 0.2])),
              E.RayTracingMesh(E.Mesh(pos[half:], np.arange(len(pos) - half, dtype=np.uint32)),
                               E.MetalMaterial([0.6, 0.6, 0.9], 0.8, 0.1))]
    return E.RayTracerSettings(num_samples=SPP, max_bounces=BOUNCES, use_environment_lighting=True, mesh_data=meshes,
                               up=camera.up)


@functools.lru_cache(maxsize=None)
def make_case(name, cam):
    scene, size = SCENES[name]
    if name == "needle":
        # the slivers are built for the first camera; the second sees them from elsewhere (ordinary thin triangles)
        camera = E.Camera(*NEEDLE_CAMERA)
        case = SceneCase(None, size, SPP, BOUNCES, settings=needle_settings(camera, size), camera=camera)
    else:
        case = SceneCase(scene, size, SPP, BOUNCES)
    if CAMERAS[name][cam] is not None:
        case.camera = E.Camera(*CAMERAS[name][cam])
    return case


@functools.lru_cache(maxsize=None)
def gpu_lists(name, cam):
    """((n, ok, entries) of refine = 0, the same of refine = 1, tiles per row)."""
    case = make_case(name, cam)
    ctx = case.context(variant=WQ)
    pc = case.push(1)
    n0, ok0, e0, tx = ctx.tile_lists(pc, refine=False)
    n1, ok1, e1, _ = ctx.tile_lists(pc, refine=True)
    ctx.close()
    return (n0, ok0, e0), (n1, ok1, e1), tx


@functools.lru_cache(maxsize=None)
def truth(name, cam):
    case = make_case(name, cam)
    return model.tile_hits(case.push(1), case.rays, case.tris, case.meshes)


@functools.lru_cache(maxsize=None)
def oracle_frames(name, cam, rows=None):
    case = make_case(name, cam)
    return tuple(pyoracle.trace(case.push(k), case.rays, case.spheres, case.tris, case.meshes, rows=rows)
                 for k in (1, 2, 3))


def assert_sound(name, cam, lists, what, skip_limit=0.05):
    n, ok, ent = lists
    hit = truth(name, cam)
    assert len(hit) == len(n)
    skipped = 0
    for t, want in enumerate(hit):
        if not ok[t]:
            skipped += 1  # the kernels cull such a tile per iteration: it has no list to be wrong
            continue
        missing = np.setdiff1d(want, ent[t, :n[t]])
        assert missing.size == 0, f"{name} camera {cam} tile {t} ({what}): hit triangles {missing.tolist()} not listed"
    assert skipped <= skip_limit * len(n), f"{skipped} of {len(n)} tiles overflowed"
    return sum(1 for w in hit if w.size)


@pytest.mark.parametrize("name,cam", CASES)
def test_every_hit_triangle_is_listed(name, cam):
    """Soundness, direct: every triangle that a float64 Moller-Trumbore test finds hit (u, v, w >= 1e-4, t > 0.001)
    by a pixel's jitter-box corner rays, its centre ray or 8 seeded rays inside the box -- float32 directions as
    get_ray_dir forms them -- is in the pixel's tile list.  Tiles without a list (ok = 0) are skipped, at most 5% of
    the tiles; the cap rule's own lists (refine = 0) are held to the same truth wherever they exist (more of them
    overflow: that is the rule this one replaces, so no limit there)."""
    l0, l1, _ = gpu_lists(name, cam)
    tiles_hit = assert_sound(name, cam, l1, "refine = 1")
    assert_sound(name, cam, l0, "refine = 0", skip_limit=1.0)
    assert tiles_hit > 0  # the camera sees geometry: the test has something to find


@pytest.mark.parametrize("name,cam", LIST_CASES)
def test_refined_lists_are_ordered_sublists(name, cam):
    """Per tile, the refined list is a sub-sequence of the cap rule's list (same order), and a tile whose cap-rule
    list fits still fits; on island 192x108 strictly fewer tiles keep a list."""
    (n0, ok0, e0), (n1, ok1, e1), _ = gpu_lists(name, cam)
    for t in range(len(n0)):
        if not ok0[t]:
            continue
        assert ok1[t]
        a, b = e0[t, :n0[t]].tolist(), e1[t, :n1[t]].tolist()
        it = iter(a)
        assert all(x in it for x in b), f"tile {t}: {b} is not a sub-sequence of {a}"
    if name == "island":
        # tiles the planner cannot hand to the sky lane: a list with entries, or no list at all
        assert np.count_nonzero(~ok1 | (n1 > 0)) < np.count_nonzero(~ok0 | (n0 > 0))

@pytest.mark.parametrize("name,cam", LIST_CASES)
def test_lists_equal_the_model(name, cam):
    """Both rules against tools/tile_cull_model.py in the kernel's float32 arithmetic: the same entries in the same
    order, except entries some comparison of which lies within 1e-4 (relative) of its threshold in the model."""
    case = make_case(name, cam)
    l0, l1, _ = gpu_lists(name, cam)
    for (n, ok, ent), rule in ((l0, "cap"), (l1, "pixel")):
        m = model.tile_lists(case.push(1), case.rays, case.tris, case.meshes, rule=rule, mirror=True)
        for t in range(len(n)):
            border = m["border"][t]
            if bool(ok[t]) != m["ok"][t]:
                assert border, f"{rule} tile {t}: ok {ok[t]} vs the model's {m['ok'][t]} with no borderline entry"
                continue
            if not ok[t]:
                continue
            got = [k for k in ent[t, :n[t]].tolist() if k not in border]
            want = [k for k in m["lists"][t].tolist() if k not in border]
            assert got == want, f"{rule} tile {t}: {got} vs the model's {want}"


def render(case, frames, script, partition=None, options=None):
    """script: "n" = one hrt_compute_n of 3 frames, "loop" = 3 x (hrt_trace, hrt_accumulate), in order, each after a
    clear; every pass's accumulator, last trace image and counters against the oracle's frames 1..3."""
    ctx = case.context(variant=WQ, partition=partition, options=options)
    rows = ctx.global_rows()
    real = rows < ctx.height
    acc = np.zeros_like(frames[0][0])
    pyoracle.accumulate_rgba8(0, acc, acc.copy())
    for k in (1, 2, 3):
        pyoracle.accumulate_rgba8(k, acc, frames[k - 1][0])
    for kind in script:
        ctx.reset_stats()
        ctx.trace(case.push(0, init=True))
        ctx.accumulate(0)
        if kind == "n":
            ctx.compute_n(case.push(1), 3)
        else:
            for k in (1, 2, 3):
                ctx.trace(case.push(k))
                ctx.accumulate(k)
        st = ctx.stats()
        got = ctx.read(_lib.IMG_ACCUM)[real]
        assert np.array_equal(got, acc[rows[real]]), f"{kind}: accumulator " + mismatch_report(got, acc[rows[real]])
        got, want = ctx.read(_lib.IMG_TRACE)[real], frames[2][0][rows[real]]
        assert np.array_equal(got, want), f"{kind}: frame 3 " + mismatch_report(got, want)
        yield st
    ctx.close()


@pytest.mark.parametrize("name,cam", CASES)
def test_frames_equal_the_oracle(name, cam):
    """3 frames in one hrt_compute_n and as the per-frame loop: images byte for byte, segments and triangle tests
    equal (the later passes follow a plan: tiles with an empty list are sky items)."""
    case = make_case(name, cam)
    frames = oracle_frames(name, cam)
    for st in render(case, frames, ("n", "loop", "n")):
        assert (st.segments, st.tri_tests) == (sum(f[2] for f in frames), sum(f[3] for f in frames))


@pytest.mark.parametrize("name", ["island", "needle"])
def test_split_tiles_build_their_lists_in_the_kernel(name):
    """HRT_OPT_SPLIT = 8 with every tile heavy (HRT_OPT_SPLIT_FACTOR = 0): planned passes run each tile as row
    groups, whose items build their list in the kernel from their own active lanes."""
    case = make_case(name, 0)
    frames = oracle_frames(name, 0)
    for st in render(case, frames, ("loop", "n", "loop"), options={_lib.OPT_SPLIT: 8, _lib.OPT_SPLIT_FACTOR: 0}):
        assert (st.segments, st.tri_tests) == (sum(f[2] for f in frames), sum(f[3] for f in frames))


@pytest.mark.parametrize("part", [0, 1])
def test_row_tile_partition_of_two(part):
    """A 2-part row-tile partition (row tile 4: every 8-row tile of a part spans two global row tiles, and the
    ragged image's last tile has padding rows): real rows against the oracle's."""
    case = make_case("ragged", 0)
    frames = oracle_frames("ragged", 0)
    for _ in render(case, frames, ("n", "loop", "n"), partition=(4, part, 2),
                    options={_lib.OPT_SPLIT: 8, _lib.OPT_SPLIT_FACTOR: 0}):
        pass
