"""The variance-guided denoise's numpy reference (tests/variance_ref.py) on the CPU: the
properties S16 implies, and the quality conditions of the defaults on oracle frames -- after a camera move, the
variance-guided filter over the reprojected history is closer to the oracle's 256-frame accumulation than the
unfiltered accumulator after 1, 2 and 4 new frames, closer than the fixed-sigma filter (S14) after 1 and 4, and on a
settled 16-frame history it changes the image less than S14 does (DESIGN.md §31 has the grid the defaults come from)."""
import numpy as np
import pytest

import denoise_ref as D
import history_ref as H
import image_ref as I
import variance_ref as V
from epq_raytracer_amd import _lib
from image_ref import same_floats
from test_history_ref import make_hits, oracle_move

F32 = np.float32


def bits_equal(a, b):
    return bool(same_floats(a, b).all())


def counts_and_moments(rng, h, w, lo=4, hi=20):
    cnt = rng.integers(lo, hi, (h, w)).astype(np.uint32)
    m1 = rng.uniform(0, 2, (h, w)).astype(F32)
    mom = np.stack([m1, m1 * m1 + rng.uniform(0, 0.5, (h, w)).astype(F32)], -1)
    return cnt, mom


def test_defaults_are_the_headers():
    assert V.DEFAULTS[:3] == (_lib.VARIANCE_SIGMA, _lib.VARIANCE_FLOOR, _lib.VARIANCE_MIN_HISTORY)
    assert V.DEFAULTS[3:] == D.DEFAULT_SIGMAS[1:]


def test_a_constant_image_passes_unchanged_and_its_variance_shrinks_by_the_weights():
    rng = np.random.default_rng(3)
    h, w = 23, 37
    cnt, mom = counts_and_moments(rng, h, w)
    acc = np.ones((h, w, 4), F32)
    acc[..., :3] = (0.5, 0.25, 0.75)  # dyadic: every product with a kernel weight is exact
    out, _ = V.denoise_variance(acc, cnt, mom, 5)
    assert bits_equal(out, acc)
    any_colour = np.ones((h, w, 4), F32)
    any_colour[..., :3] = (0.3, 1.7, 0.011)
    out, _ = V.denoise_variance(any_colour, cnt, mom, 5)
    assert np.allclose(out, any_colour, rtol=1e-6, atol=0)
    # every colour weight is 1, so w is the B3 kernel alone: V' = sum(w^2 V(q)) / (sum w)^2
    c = V.source_colour(acc)
    v = V.variance_estimate(c, cnt, mom, np.zeros((h, w), np.uint32), 4)
    assert np.isfinite(v).all() and (v > 0).any()
    k1 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    for i in range(3):
        s = 1 << i
        _, v2 = V.one_pass(c, v, i, *V.DEFAULTS[:2], *V.DEFAULTS[3:])
        assert np.isfinite(v2).all()
        y, x = h // 2, w // 2  # (every tap of the centre pixel is inside the image at steps 1, 2, 4)
        taps = v[y - 2 * s:y + 2 * s + 1:s, x - 2 * s:x + 2 * s + 1:s].astype(np.float64)
        w2 = np.outer(k1, k1)
        assert np.isclose(v2[y, x], (w2 * w2 * taps).sum() / w2.sum() ** 2, rtol=1e-5)
        # a uniform variance shrinks by sum(w^2) / (sum w)^2 wherever every tap is inside
        _, u2 = V.one_pass(c, np.full((h, w), 0.5, F32), i, *V.DEFAULTS[:2], *V.DEFAULTS[3:])
        assert np.isclose(u2[y, x], 0.5 * (w2 * w2).sum() / w2.sum() ** 2, rtol=1e-5)
        v = v2


def test_moments_of_a_constant_signal_give_zero_variance():
    h, w = 9, 11
    c = F32(0.7)
    mom = np.empty((h, w, 2), F32)
    mom[..., 0], mom[..., 1] = c, c * c
    acc = np.random.default_rng(1).uniform(0, 2, (h, w, 4)).astype(F32)
    for n in (4, 5, 1 << 24):
        v0 = V.variance_estimate(V.source_colour(acc), np.full((h, w), n, np.uint32), mom, np.zeros((h, w), np.uint32), 4)
        assert (v0 == 0).all()
    # negative estimates (m2 below m1^2 by rounding) clamp to 0
    mom[..., 1] = c * c - F32(1e-3)
    assert (V.variance_estimate(V.source_colour(acc), np.full((h, w), 9, np.uint32), mom, np.zeros((h, w), np.uint32), 4) == 0).all()


@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_the_moments_fold(dtype):
    rng = np.random.default_rng(8)
    h, w = 6, 9
    if dtype == np.uint8:
        acc, new = (rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(2))
    else:
        acc, new = (rng.uniform(0, 4, (h, w, 4)).astype(F32) for _ in range(2))
    # k identical frames: (l, l*l) to rounding, counts 1..k
    cnt, mom = np.zeros((h, w), np.uint32), np.full((h, w, 2), np.nan, F32)  # (the old M is not read at n == 0)
    a = np.zeros_like(acc)
    l = V.lum(V.source_colour(new))
    for k in range(6):
        a, cnt, mom = V.accumulate_history_moments(a, cnt, mom, new, 32)
        if k == 0:
            assert bits_equal(mom[..., 0], l) and bits_equal(mom[..., 1], l * l)
        assert np.allclose(mom[..., 0], l, rtol=1e-6) and np.allclose(mom[..., 1], l * l, rtol=1e-6)
    assert (cnt == 6).all()
    # mixed counts, the cap, 2^24 and the count whose successor wraps: fold_rgba32f on the two channels
    cnt = rng.integers(0, 5, (h, w)).astype(np.uint32)
    cnt[0, :5] = [1 << 24, (1 << 24) - 1, 31, 32, 2**32 - 1]
    mom = rng.uniform(0, 3, (h, w, 2)).astype(F32)
    acc2, cnt2, mom2 = V.accumulate_history_moments(acc, cnt, mom, new, 32)
    wa, wc = H.accumulate_history(acc, cnt, new, 32)
    assert acc2.tobytes() == wa.tobytes() and np.array_equal(cnt2, wc)
    for y in range(h):
        for x in range(w):
            n = int(cnt[y, x])
            sample = np.array([l[y, x], l[y, x] * l[y, x], 0, 0], F32)
            if n == 0:
                want = sample[:2]
            else:
                cur4 = np.array([mom[y, x, 0], mom[y, x, 1], 0, 0], F32)
                want = I.fold_rgba32f(n, cur4[None], sample[None])[0, :2]
            assert bits_equal(mom2[y, x], want), (x, y, n)
    assert np.isinf(mom2[0, 4]).all()  # frame + 1 wrapped to 0: IEEE's division by zero


@pytest.mark.parametrize("name", ["box", "spheres"])
def test_moments_through_the_reprojection(name):
    (vp, vc), (hp, hc), *_ = oracle_move(name)
    rng = np.random.default_rng(12)
    h, w = hp.shape
    acc = rng.uniform(0, 4, (h, w, 4)).astype(F32)
    cnt = rng.integers(0, 3, (h, w)).astype(np.uint32) * 7
    mom = rng.uniform(0.5, 3, (h, w, 2)).astype(F32)
    mom[3, 4], cnt[3, 4] = (np.nan, -0.0), 9
    # the identity view with NEAREST: bit for bit where there is history, (0, 0) where there is none
    a2, c2, m2 = V.reproject_moments(acc, cnt, mom, vp, hp, vp, hp, H.NEAREST)
    wa, wc = H.reproject(acc, cnt, vp, hp, vp, hp, H.NEAREST)
    assert bits_equal(a2, wa) and np.array_equal(c2, wc) and np.array_equal(c2, cnt)
    held = cnt > 0
    assert bits_equal(m2[held], mom[held]) and (m2[~held].view(np.uint32) == 0).all()
    # the move: a rejected pixel has M' = (0, 0); a carried one a weighted mean of its taps' moments
    for filt in (H.NEAREST, H.BILINEAR):
        a2, c2, m2 = V.reproject_moments(acc, np.full((h, w), 5, np.uint32), mom, vp, hp, vc, hc, filt)
        rejected = c2 == 0
        assert rejected.any() and (~rejected).any()
        assert (m2[rejected].view(np.uint32) == 0).all()
        ok = ~rejected & ~np.isnan(m2).any(-1)
        assert (m2[ok] >= 0.5 - 1e-5).all() and (m2[ok] <= 3 + 1e-5).all()


def test_the_spatial_estimate_skips_other_keys_and_the_outside():
    h, w = 5, 7  # smaller than the 7 x 7 window in both axes
    rng = np.random.default_rng(4)
    c = rng.uniform(0, 2, (h, w, 3)).astype(F32)
    cnt, mom = np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    key = np.zeros((h, w), np.uint32)
    key[:, 4:] = 9
    v0 = V.variance_estimate(c, cnt, mom, key, 4)
    lq = V.lum(c)
    for y in range(h):
        for x in range(w):
            s1 = s2 = k = F32(0)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    qy, qx = y + dy, x + dx
                    if not (0 <= qy < h and 0 <= qx < w) or key[qy, qx] != key[y, x]:
                        continue
                    s1, s2, k = s1 + lq[qy, qx], s2 + lq[qy, qx] * lq[qy, qx], k + F32(1)
            mean = s1 / k
            e = s2 / k - mean * mean
            assert bits_equal(v0[y, x], e if e > 0 else F32(0)), (x, y)
    # changing a pixel of the other key, or the moments, leaves the estimates of this key alone
    c2 = c.copy()
    c2[2, 5] += F32(1)
    v1 = V.variance_estimate(c2, cnt, mom + F32(3), key, 4)
    assert bits_equal(v1[:, :4], v0[:, :4]) and not bits_equal(v1[:, 4:], v0[:, 4:])
    # counts at min_history take the temporal estimate, below it the spatial one
    cnt[1, 1], cnt[1, 2] = 4, 3
    mom[1, 1] = mom[1, 2] = (1.0, 3.0)
    v2 = V.variance_estimate(c, cnt, mom, key, 4)
    assert v2[1, 1] == F32(0.5) and bits_equal(v2[1, 2], v0[1, 2])
    # a single pixel of its key: k = 1, variance 0
    lone = np.zeros((1, 1), np.uint32)
    assert V.variance_estimate(c[:1, :1], lone, mom[:1, :1], lone, 4)[0, 0] == 0


def test_iterations_zero_returns_the_source_and_the_estimate():
    rng = np.random.default_rng(6)
    h, w = 7, 5
    acc = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    cnt, mom = counts_and_moments(rng, h, w, 0, 9)
    hits = make_hits(h, w, kind=2, mesh=0, index=1, t=2.0, normal=(0.0, 0.0, 1.0))
    out, v = V.denoise_variance(acc, cnt, mom, 0, hits=hits, fmt_rgba8=True)
    assert out[..., :3].tobytes() == acc[..., :3].tobytes() and (out[..., 3] == 255).all()
    assert bits_equal(v, V.variance_estimate(V.source_colour(acc), cnt, mom, np.ones((h, w), np.uint32), 4))


# ---- the quality conditions of the defaults -----------------------------------------------------------------------

def history_with_moments(frames, max_history=32):
    h, w = frames[0].shape[:2]
    acc, cnt, mom = np.zeros_like(frames[0]), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    for f in frames:
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, f, max_history)
    return acc, cnt, mom


@pytest.mark.parametrize("name", ["box", "spheres"])
def test_variance_guided_filter_beats_the_accumulator_and_the_fixed_sigma_filter_after_the_move(name):
    (vp, vc), (hp, hc), old, new, target = oracle_move(name)
    tgt = target[..., :3].astype(np.float64)

    def mse(a):
        return float(((a[..., :3] - tgt) ** 2).mean())

    acc, cnt, mom = history_with_moments(old)
    assert (cnt == 16).all()
    acc, cnt, mom = V.reproject_moments(acc, cnt, mom, vp, hp, vc, hc, H.BILINEAR, *H.DEFAULTS)
    for k, frame in enumerate(new, 1):
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, frame, 32)
        if k not in (1, 2, 4):
            continue
        guided = mse(V.denoise_variance(acc, cnt, mom, 5, V.DEFAULTS, hits=hc)[0])
        fixed = mse(D.denoise(acc, 5, hits=hc))
        print(f"{name} k={k}: mse unfiltered {mse(acc):.6f}, S14 {fixed:.6f}, variance-guided {guided:.6f}")
        assert guided < mse(acc)  # (a)
        if k != 2:  # (b); k = 2 is recorded above, not asserted (spheres is within 3 % there)
            assert guided < fixed


@pytest.mark.parametrize("name", ["box", "spheres"])
def test_variance_guided_filter_leaves_a_settled_history_more_nearly_alone(name):
    _, (hp, _), old, _, _ = oracle_move(name)
    acc, cnt, mom = history_with_moments(old)
    guided = V.denoise_variance(acc, cnt, mom, 5, V.DEFAULTS, hits=hp)[0]
    fixed = D.denoise(acc, 5, hits=hp)
    dg, df = (float(np.abs(o[..., :3] - acc[..., :3]).mean()) for o in (guided, fixed))
    print(f"{name}: mean |out - in| variance-guided {dg:.6f}, S14 {df:.6f}")
    assert dg < df  # (c)
