"""The radiance queries' reference on the CPU (tests/radiance_ref.py): orc_trace_pixel on a 1 x 1 image with
cam_pos = origin, rays[0] = centre and rng_offset = seed * 719393^-1 reproduces whole oracle frames -- every
pixel of a 32 x 32 frame at 2 samples and 4 bounces as the query (cam_pos, rng_offset * 719393 + id, centre id),
rgb before quantisation and the frame's segment and triangle-test counts."""
import numpy as np
import pytest

import radiance_ref as R
from helpers import SceneCase


def test_seed_map_is_a_bijection():
    assert R.SEED_MUL % 2 == 1 and R.SEED_MUL * R.SEED_INV % (1 << 32) == 1
    for seed in (0, 1, 0xFFFFFFFF, 719393, 123456789):
        assert (seed * R.SEED_INV % (1 << 32)) * R.SEED_MUL % (1 << 32) == seed


@pytest.mark.parametrize("name", ["island", "box", "cave", "spheres"])
def test_construction_reproduces_oracle_frames(name):
    case = SceneCase(name, (32, 32), 2, 4)
    pc = case.push(3)
    _, frame, segments, tri_tests = case.oracle(3, want_f32=True)
    ids = np.arange(32 * 32)
    queries = R.pixel_queries(case, pc, ids % 32, ids // 32)
    assert (queries["seed"] == (3 * 719393 + ids) % (1 << 32)).all()
    # pc's own camera position, image size and rng_offset must not matter to the construction
    other = R.copy_push(pc, rng_offset=77, width=5, height=9)
    other.cam_pos[0] = 123.0
    rgba, seg, tests = R.oracle(case, other, queries)
    assert R.same_bits(rgba, frame.reshape(-1, 4)), R.explain(rgba, frame.reshape(-1, 4), queries)
    assert (int(seg.sum()), int(tests.sum())) == (segments, tri_tests)
    assert (seg > 2).sum() > 100  # paths that bounce (the camera family alone: 118 of 1,024 on island)


def test_families_are_seeded_and_flag_the_irregular():
    case = SceneCase("box", (37, 23), 1, 1)
    import query_ref as Q
    qs = Q.QueryScene(case)
    pc = case.push()
    a, b = R.families(case, qs, pc, 64, 5), R.families(case, qs, pc, 64, 5)
    assert list(a) == ["camera", "surface", "far", "seeds", "irregular"]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes()
    assert set(a["seeds"]["seed"]) == {0, 0xFFFFFFFF}
    irr = R.always_irregular(a["irregular"])
    assert irr.sum() == len(irr) * 4 // 5 and not R.always_irregular(a["far"]).any()
    # the far origins are 1e3 and 1e6 scene diagonals from the scene
    d = np.linalg.norm(a["far"]["origin"].astype(np.float64) - qs.centre, axis=1) / qs.diagonal
    assert (d[0::2] > 5e2).all() and (d[0::2] < 2e3).all() and (d[1::2] > 5e5).all()
