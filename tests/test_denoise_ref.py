"""The denoise pass's numpy reference (tests/denoise_ref.py) on the CPU: the properties S14
implies, and the quality condition of the default sigmas on 1-spp oracle frames -- the filtered frame is closer
to the oracle's 256-frame accumulation than the unfiltered one (DESIGN.md §27 has the grid the sigmas come from)."""
import functools

import numpy as np
import pytest

import denoise_ref as D
import pyoracle
import query_ref as Q
from epq_raytracer_amd import _lib
from helpers import SceneCase
from image_ref import same_floats

F32 = np.float32
FLT_MAX = np.finfo(F32).max


def make_hits(h, w, kind=2, mesh=0, index=0, t=1.0, normal=(0.0, 0.0, 1.0)):
    hits = np.zeros((h, w), dtype=_lib.HIT_DTYPE)
    hits["kind"], hits["mesh"], hits["index"], hits["t"], hits["normal"] = kind, mesh, index, t, normal
    return hits


def test_surface_keys():
    hits = np.zeros(5, dtype=_lib.HIT_DTYPE)
    hits["kind"] = [0, 1, 2, 2, 3]
    hits["index"] = [0xFFFFFFFF, 0x80000005, 7, 7, 1]
    hits["mesh"] = [0xFFFFFFFF, 0xFFFFFFFF, 0, 0x7FFFFFFF, 1]
    assert D.surface_keys(hits).tolist() == [0, 0x80000005, 1, 0, 0]


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("value", [0.0, 1.0])
def test_constant_images_are_fixed_points(value, guided):
    img = np.full((9, 11, 4), value, F32)
    hits = make_hits(9, 11) if guided else None
    out = D.denoise(img, 5, hits=hits)
    assert out.tobytes() == np.concatenate([img[..., :3], np.ones((9, 11, 1), F32)], -1).tobytes()
    img8 = np.full((9, 11, 4), int(value * 255), np.uint8)
    out8 = D.denoise(img8, 3, hits=hits, fmt_rgba8=True)
    assert (out8[..., :3] == int(value * 255)).all() and (out8[..., 3] == 255).all()


def test_taps_across_a_key_boundary_contribute_nothing():
    h, w = 12, 20
    img = np.zeros((h, w, 4), F32)
    # powers of two: w * c is exact, so (sum of w * c) / (sum of w) is c whatever the weights are
    img[:, :9, :3], img[:, 9:, :3] = (0.25, 0.5, 1.0), (4.0, 0.125, 0.0)
    hits = make_hits(h, w)
    hits["mesh"][:, 9:] = 5
    hits["kind"][:4, 9:], hits["index"][:4, 9:] = 1, 3  # a sphere region inside the right half, same colour
    out = D.denoise(img, 5, hits=hits)
    assert out[..., :3].tobytes() == img[..., :3].tobytes()
    # without the guide the regions bleed into each other
    assert D.denoise(img, 5)[..., :3].tobytes() != img[..., :3].tobytes()


def test_one_pixel_image_returns_itself():
    img = np.array([[[0.3, 7.0, 0.0, 0.5]]], F32)
    for hits in (None, make_hits(1, 1), make_hits(1, 1, kind=0, t=FLT_MAX, normal=(0, 0, 0))):
        out = D.denoise(img, 5, hits=hits)
        assert out[0, 0, :3].tobytes() == img[0, 0, :3].tobytes() and out[0, 0, 3] == 1.0


def test_nan_stays_and_spreads_only_within_its_key():
    h, w = 40, 40
    rng = np.random.default_rng(3)
    img = rng.uniform(0, 1, (h, w, 4)).astype(F32)
    hits = make_hits(h, w)
    hits["mesh"][:, 20:] = 1
    img[10, 10, 1] = np.nan
    out = D.denoise(img, 5, hits=hits)
    assert np.isnan(out[10, 10, :3]).all()  # every weight of the NaN pixel's taps is NaN
    assert np.isnan(out[:, :20, :3]).any(axis=-1).sum() > 1
    assert not np.isnan(out[:, 20:]).any()
    # a NaN normal: the comparison rule gives weight 0, not NaN -- the tap is dropped, nothing is poisoned
    hits2 = make_hits(h, w)
    hits2["normal"][5, 5] = (np.nan, 0, 0)
    img2 = rng.uniform(0, 1, (h, w, 4)).astype(F32)
    out2 = D.denoise(img2, 1, hits=hits2)
    assert np.isnan(out2[5, 5, :3]).all()  # its own taps all weigh 0: 0 / 0
    assert np.isnan(out2[..., :3]).any(axis=-1).sum() == 1


@functools.lru_cache(maxsize=None)
def oracle_frames(name):
    """(1-spp frame, the oracle's accumulation of 256 frames, first hits) of a 64 x 64 RGBA32F render, 8 bounces."""
    case = SceneCase(name, (64, 64), num_samples=1, max_bounces=8, rng_offset=1)
    acc = np.zeros((64, 64, 4), F32)
    noisy = None
    for k in range(256):
        frame = case.oracle(rng_offset=1 + k, want_f32=True)[1]
        noisy = frame.copy() if k == 0 else noisy
        pyoracle.accumulate_rgba32f(k, acc, frame)
    ys, xs = np.mgrid[0:64, 0:64]
    hits = Q.QueryScene(case).hits(Q.primary_rays(case, case.push(), xs.reshape(-1), ys.reshape(-1)))[0]
    return noisy, acc, hits.reshape(64, 64)


@pytest.mark.parametrize("name", ["box", "spheres"])
def test_default_sigmas_reduce_the_error_of_a_one_sample_frame(name):
    noisy, target, hits = oracle_frames(name)
    assert D.DEFAULT_SIGMAS == _lib.DENOISE_SIGMAS
    out = D.denoise(noisy, 5, D.DEFAULT_SIGMAS, hits)
    tgt = target[..., :3].astype(np.float64)
    mse_raw = float(((noisy[..., :3] - tgt) ** 2).mean())
    mse_out = float(((out[..., :3] - tgt) ** 2).mean())
    print(f"{name}: mse unfiltered {mse_raw:.6f}, filtered {mse_out:.6f}")
    assert mse_out < mse_raw
    assert same_floats(out[..., 3], np.ones((64, 64), F32)).all()
