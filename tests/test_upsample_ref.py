"""Guided upsampling on the CPU: the HIP-free coordinate header the upsample kernel shares
(epq_raytracer_amd/csrc/hrt_upsample_map.h), compiled into a stand-alone program (tests/cpp/upsample_map_test.cpp,
-ffp-contract=off; once more under AddressSanitizer and UBSan), against the numpy restatement tests/upsample_ref.py
word for word; then properties of the restatement itself."""
import os
import subprocess

import numpy as np
import pytest

import upsample_ref as U
from epq_raytracer_amd import _lib
from image_ref import same_floats

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
F32 = np.float32
N = 48
EXTRA = [(960, 1920), (1920, 3840), (540, 1080), (16384, 16384), (1, 16384), (16384, 1), (1000, 16383), (1 << 24, 7)]


def build(target):
    subprocess.run(["make", "-s", "-C", CPP, "-f", "upsample_demo.mk", target], check=True)
    return os.path.join(CPP, target)


def expected_words(pairs):
    """The program's output for (ws, wt) pairs, from the restatement: eleven words per footprint, pair and x."""
    out = []
    for footprint in (2, 4):
        for ws, wt in pairs:
            u, x0, taps = U.axis_taps(wt, ws, footprint)
            rec = np.zeros((wt, 11), np.uint32)
            rec[:, 0], rec[:, 1], rec[:, 2] = u.view(np.uint32), x0.view(np.uint32), U.nearest(wt, ws)
            for slot, (_, inside, w) in enumerate(taps):
                rec[:, 3 + 2 * slot], rec[:, 4 + 2 * slot] = inside, w.view(np.uint32)
            out.append(rec)
    return np.concatenate(out)


@pytest.mark.parametrize("target", ["upsample_map_test", "upsample_map_test_san"])
def test_header_matches_the_restatement_bit_for_bit(target):
    """Every (Ws, Wt) in 1..48 x 1..48 and every x, both footprints: x0, the bounds tests, the weights and the
    fallback's sx; plus the sizes the rates are measured at and the largest ones."""
    args = [str(N)] + [str(v) for p in EXTRA for v in p]
    r = subprocess.run([build(target)] + args, capture_output=True, timeout=600)
    assert r.returncode == 0 and b"ERROR" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:]
    got = np.frombuffer(r.stdout, np.uint32).reshape(-1, 11)
    want = expected_words([(ws, wt) for ws in range(1, N + 1) for wt in range(1, N + 1)])
    # (the program emits the grid and then the extra pairs per footprint)
    grid = len(want) // 2
    extra = expected_words(EXTRA)
    half = len(extra) // 2
    want = np.concatenate([want[:grid], extra[:half], want[grid:], extra[half:]])
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[0], got[bad[0][0]], want[bad[0][0]])


# ---- properties of the restatement ------------------------------------------------------------------------------

def guide(h, w, seed=3, blocks=True):
    """Hit records: blocky keys (misses, spheres, triangles), unit normals, depths with equal values."""
    rng = np.random.default_rng([seed, w, h])
    hits = np.zeros((h, w), dtype=_lib.HIT_DTYPE)
    by, bx = np.mgrid[0:h, 0:w]
    block = rng.integers(0, 6, ((h + 3) // 4, (w + 4) // 5))[by // 4, bx // 5] if blocks else np.zeros((h, w), np.int64)
    hits["kind"] = np.choose(block % 3, [0, 1, 2])
    hits["index"] = np.where(hits["kind"] == 0, 0xFFFFFFFF, block + 3)
    hits["mesh"] = np.where(hits["kind"] == 2, block // 3, 0xFFFFFFFF)
    n = rng.normal(size=(h, w, 3))
    hits["normal"] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    hits["t"] = np.where(hits["kind"] == 0, np.finfo(F32).max, np.round(rng.uniform(1, 9, (h, w)) * 4) / 4)
    return hits


def image(h, w, seed=4):
    return (np.random.default_rng([seed, w, h]).uniform(0, 1, (h, w, 4)) ** 2 * 4).astype(F32)


@pytest.mark.parametrize("footprint", [2, 4])
def test_equal_sizes_with_the_same_guide_reproduce_the_image(footprint):
    """Wt = Ws: u is the pixel's own index and its own tap has h = 1.  Footprint 2's other taps have weight 0, so the
    image comes back bit for bit on any guide whose own-tap weights are 1; footprint 4's neighbours weigh 0.5, so it
    comes back where they are of another surface -- here every pixel is a surface of its own."""
    h, w = 11, 13
    low, hits = image(h, w), guide(h, w)
    hits["normal"] = (0.0, 0.0, 1.0)  # the own tap's wn = wd = 1 exactly
    if footprint == 4:
        hits["kind"], hits["index"] = 1, np.arange(h * w).reshape(h, w)
        hits["t"] = 2.5
    out, kept, fallback = U.upsample(low, hits, hits, footprint, with_info=True)
    assert not fallback.any() and (kept == 1).all()
    assert same_floats(out[..., :3], low[..., :3]).all() and (out[..., 3] == 1).all()
    # ... and with one surface everywhere footprint 4 does blur, footprint 2 still does not
    hits["kind"], hits["index"], hits["t"] = 1, 7, 2.5
    out, kept, _ = U.upsample(low, hits, hits, footprint, with_info=True)
    if footprint == 2:
        assert (kept == 1).all() and same_floats(out[..., :3], low[..., :3]).all()
    else:
        assert kept.max() == 9 and kept.min() == 4 and not same_floats(out[..., :3], low[..., :3]).all()


@pytest.mark.parametrize("footprint", [2, 4])
@pytest.mark.parametrize("size", [(7, 5, 14, 10), (7, 5, 19, 8), (16, 16, 8, 8), (1, 1, 3, 2)])
def test_a_constant_image_stays_constant(size, footprint):
    ws, hs, wt, ht = size
    low = np.full((hs, ws, 4), F32(0.625))
    out, kept, fallback = U.upsample(low, guide(hs, ws, blocks=False), guide(ht, wt, blocks=False), footprint,
                                     with_info=True)
    # constant up to rounding: with n = footprint^2 positive terms, acc carries at most n roundings (a product and an
    # add per tap), wsum n - 1 and the division one: a relative error of at most (2 n + 1) 2^-24 to first order
    bound = (2 * footprint * footprint + 1) * 2.0 ** -24 * 0.625
    assert np.abs(out[..., :3].astype(np.float64) - 0.625).max() <= bound and (out[..., 3] == 1).all()
    assert (kept >= 1).all() and not fallback.any()


@pytest.mark.parametrize("size", [(7, 5, 14, 10), (7, 5, 19, 8), (9, 4, 5, 3)])
def test_an_all_miss_guide_gives_plain_bilinear_weights(size):
    """Every key 0: wn = wd = 1, so footprint 2 is the bilinear interpolation with the edge taps dropped and the
    rest renormalised."""
    ws, hs, wt, ht = size
    low = image(hs, ws)
    miss_lo, miss_hi = np.zeros((hs, ws), _lib.HIT_DTYPE), np.zeros((ht, wt), _lib.HIT_DTYPE)
    out = U.upsample(low, miss_lo, miss_hi, 2)
    want = np.zeros((ht, wt, 3), np.float64)
    for y in range(ht):
        for x in range(wt):
            u, v = (x + 0.5) * ws / wt - 0.5, (y + 0.5) * hs / ht - 0.5
            x0, y0 = int(np.floor(u)), int(np.floor(v))
            acc, wsum = np.zeros(3), 0.0
            for yj in (y0, y0 + 1):
                for xj in (x0, x0 + 1):
                    wgt = (1 - abs(u - xj)) * (1 - abs(v - yj))
                    if 0 <= xj < ws and 0 <= yj < hs and wgt > 0:
                        acc += wgt * low[yj, xj, :3].astype(np.float64)
                        wsum += wgt
            want[y, x] = acc / wsum
    assert np.abs(out[..., :3] - want).max() < 2e-5


@pytest.mark.parametrize("footprint", [2, 4])
def test_a_pixel_whose_key_is_nowhere_in_its_footprint_takes_the_nearest_texel(footprint):
    ws, hs, wt, ht = 7, 5, 14, 10
    low = image(hs, ws)
    lo, hi = guide(hs, ws), guide(ht, wt, seed=9)
    hi["kind"][3, 4], hi["index"][3, 4] = 1, 12345  # a sphere no low texel shows
    out, kept, fallback = U.upsample(low, lo, hi, footprint, with_info=True)
    assert kept[3, 4] == 0 and fallback[3, 4]
    sx, sy = U.nearest(wt, ws)[4], U.nearest(ht, hs)[3]
    assert same_floats(out[3, 4, :3], low[sy, sx, :3]).all()
    near = U.nearest_upsample(low, wt, ht)
    assert same_floats(out[..., :3][fallback], near[fallback]).all()
