"""The adaptive refinement's numpy reference (tests/refine_ref.py) on the CPU: the properties S17
implies, and the conditions the defaults are held to on oracle frames (tools/refine_grid.py prints the whole grid,
DESIGN.md §32 keeps it): against the uniform curve -- the same frames folded for every pixel -- (a) spheres after 64
passes has a lower MSE than uniform at ceil(pixel_frames / npix) frames, (b) with at most half of uniform's 64 npix
pixel-frames, and (c) box, where every pixel is noisy, still has 85 % of its pixels selected by the 32nd pass and an
MSE within 1.1 x uniform's at floor(pixel_frames / npix) frames."""
import os
import sys

import numpy as np
import pytest

import refine_ref as R
import variance_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

F32 = np.float32
H_, W_ = 9, 13


def state(seed, h=H_, w=W_, lo=4, hi=40):
    """Counts in [lo, hi) and moments with a spread of variances, some of them 0."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(lo, hi, (h, w)).astype(np.uint32)
    m1 = rng.uniform(0.05, 2, (h, w)).astype(F32)
    spread = (rng.uniform(0, 0.2, (h, w)) * (rng.uniform(0, 1, (h, w)) < 0.7)).astype(F32)
    return cnt, np.stack([m1, m1 * m1 + spread], -1)


def test_max_count_and_min_history_take_precedence():
    cnt, mom = state(1)
    mom[..., 1] = F32(50)  # every criterion holds: the whole image would be selected
    cnt[0, :4] = [0, 3, 4, 5]
    cnt[1, :4] = [9, 10, 11, 2**32 - 1]
    sel = R.select(cnt, mom, None, 4, 10, 1, 0.05, 0.01)
    assert sel[0, :4].tolist() == [True, True, True, True]
    assert sel[1, :4].tolist() == [True, False, False, False]  # the budget
    # a settled image: only the pixels below min_history are selected, whatever they hold
    mom[..., 1] = mom[..., 0] * mom[..., 0]
    sel = R.select(cnt, mom, None, 4, 10, 1, 0.05, 0.01)
    assert sel[0, :4].tolist() == [True, True, False, False] and sel.sum() == 2
    # max_count == min_history: below it selected, from it on not -- no pixel reaches the criterion
    mom[..., 1] = F32(50)
    sel = R.select(cnt, mom, None, 4, 4, 1, 0.05, 0.01)
    assert np.array_equal(sel, cnt < 4)


@pytest.mark.parametrize("seed", [2, 3])
def test_radius_0_is_the_own_pixel_form_by_scalar_loops(seed):
    cnt, mom = state(seed, lo=0)
    key = np.random.default_rng(seed).integers(0, 3, cnt.shape).astype(np.uint32)
    for tol, fl in ((0.05, 0.01), (0.2, 0.5), (1e-3, 1e-6)):
        want = R.select_scalar_radius0(cnt, mom, 4, 30, tol, fl)
        assert np.array_equal(R.select(cnt, mom, None, 4, 30, 0, tol, fl), want)
        assert np.array_equal(R.select(cnt, mom, key, 4, 30, 0, tol, fl), want)  # the centre's key is its own


def test_other_keys_the_outside_and_short_histories_are_skipped():
    h, w = 5, 5
    cnt = np.full((h, w), 8, np.uint32)
    mom = np.zeros((h, w, 2), F32)
    mom[..., 0], mom[..., 1] = F32(1), F32(1)  # variance 0 everywhere ...
    mom[2, 2] = (1, 3)  # ... but at the centre: d = 2, se = 0.25
    key = np.zeros((h, w), np.uint32)
    # pooled over 9 kept taps: a = 0.25 / 9 = 0.0278 against tol^2 mu^2 = 0.01 (tol 0.1): the 3 x 3 block is selected
    sel = R.select(cnt, mom, key, 4, 99, 1, 0.1, 0.01)
    want = np.zeros((h, w), bool)
    want[1:4, 1:4] = True
    assert np.array_equal(sel, want)
    # the corner pixel (1, 1) keeps all nine taps; the image's corner (0, 0) would keep four, none of them noisy
    # another surface: the taps across the key boundary are skipped, so only the centre's own surface pools it
    key[:, 3:] = 7
    sel = R.select(cnt, mom, key, 4, 99, 1, 0.1, 0.01)
    want[:, 3] = False
    assert np.array_equal(sel, want)
    # with the noisy pixel on the image's edge the outside taps are not counted: (0, 0) pools 4 taps, a = 0.0625
    mom[2, 2] = (1, 1)
    mom[0, 0] = (1, 3)
    key[:] = 0
    sel = R.select(cnt, mom, key, 4, 99, 1, 0.24, 0.01)  # tol^2 = 0.0576: 0.25 / 4 passes, 0.25 / 6 and / 9 do not
    assert sel[0, 0] and sel[1, 1] == (0.25 / 9 > 0.0576) and not sel[0, 1] and sel.sum() == 1
    # a tap with a short history is skipped (its moments are not read) but is itself selected
    cnt[0, 1] = 2
    mom[0, 1] = (np.nan, np.nan)
    sel = R.select(cnt, mom, key, 4, 99, 1, 0.24, 0.01)
    # (0, 0) now pools 3 taps: 0.083; (1, 0) pools 5: 0.05 stays below tol^2
    assert sel[0, 1] and sel[0, 0] and not sel[1, 0] and sel.sum() == 2


def test_nan_and_infinite_moments_follow_the_written_comparisons():
    cnt = np.full((1, 6), 8, np.uint32)
    inf, nan = F32(np.inf), F32(np.nan)
    mom = np.array([[(nan, 1), (1, nan), (1, inf), (inf, inf), (-inf, 1), (1, 0.5)]], F32)
    sel = R.select(cnt, mom, None, 4, 99, 0, 0.05, 0.01)[0]
    # (nan, 1): d NaN -> tv 0, b NaN -> mu = floor: 0 > x false.  (1, nan): the same a = 0.
    # (1, inf): a = inf > finite.  (inf, inf): d = inf - inf = NaN -> 0.  (-inf, 1): d = -inf -> 0.  m2 < m1^2 -> 0.
    assert sel.tolist() == [False, False, True, False, False, False]
    # a NaN mean poisons its neighbours' pooled mean (b NaN -> the floor), an infinite variance their pooled a
    cnt = np.full((1, 3), 8, np.uint32)
    mom = np.array([[(1, 1), (1, inf), (1, 1)]], F32)
    assert R.select(cnt, mom, None, 4, 99, 1, 0.05, 0.01)[0].tolist() == [True, True, True]
    mom = np.array([[(1, 1.5), (nan, 1), (1, 1.5)]], F32)
    # pm = NaN -> b NaN -> mu = 0.01: a = (0.0625 + 0) / 2 > 0.0025 * 0.0001
    assert R.select(cnt, mom, None, 4, 99, 1, 0.05, 0.01)[0].tolist() == [True, True, True]


def test_a_larger_tolerance_selects_a_subset_at_radius_0():
    cnt, mom = state(5, 23, 37, lo=0)
    prev = None
    for tol in (0.01, 0.02, 0.05, 0.1, 0.2, 0.5):
        sel = R.select(cnt, mom, None, 4, 1 << 24, 0, tol, 0.01)
        if prev is not None:
            assert not (sel & ~prev).any() and sel.sum() <= prev.sum()
        prev = sel
    assert prev.sum() < R.select(cnt, mom, None, 4, 1 << 24, 0, 0.01, 0.01).sum()


def test_the_mask_layout():
    rng = np.random.default_rng(6)
    for h, w in ((1, 1), (5, 7), (23, 37), (2, 32), (4, 32)):
        sel = rng.uniform(0, 1, (h, w)) < 0.5
        sel[-1, -1] = True
        words = R.pack_mask(sel)
        assert words.dtype == np.dtype("<u4") and words.shape == ((h * w + 31) // 32,)
        for i in range(h * w):
            assert bool((int(words[i >> 5]) >> (i & 31)) & 1) == bool(sel.reshape(-1)[i])
        if (h * w) % 32:
            assert int(words[-1]) >> ((h * w) % 32) == 0  # the unused high bits of the last word
        assert np.array_equal(R.unpack_mask(words, (h, w)), sel)
        # bits beyond the image are ignored by a reader
        dirty = words.copy()
        if (h * w) % 32:
            dirty[-1] |= np.uint32((0xFFFFFFFF << ((h * w) % 32)) & 0xFFFFFFFF)
        assert np.array_equal(R.unpack_mask(dirty, (h, w)), sel)


@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_a_refinement_leaves_unselected_pixels_bytes_alone(dtype):
    rng = np.random.default_rng(7)
    h, w = 6, 11
    if dtype == np.uint8:
        acc, new = (rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(2))
    else:
        acc, new = (rng.uniform(0, 4, (h, w, 4)).astype(F32) for _ in range(2))
    cnt = rng.integers(0, 9, (h, w)).astype(np.uint32)
    mom = rng.uniform(0, 3, (h, w, 2)).astype(F32)
    mom[0, 0] = np.nan  # (kept bit for bit where unselected)
    sel = rng.uniform(0, 1, (h, w)) < 0.5
    sel[0, 0] = False
    a2, c2, m2 = R.refine(acc, cnt, mom, new, sel, 8, True)
    assert a2[~sel].tobytes() == acc[~sel].tobytes() and np.array_equal(c2[~sel], cnt[~sel])
    assert m2[~sel].tobytes() == mom[~sel].tobytes()
    wa, wc, wm = V.accumulate_history_moments(acc, cnt, mom, new, 8)
    assert a2[sel].tobytes() == wa[sel].tobytes() and np.array_equal(c2[sel], wc[sel])
    assert m2[sel].tobytes() == wm[sel].tobytes()
    # without the moments flag M keeps every byte
    a3, c3, m3 = R.refine(acc, cnt, mom, new, sel, 8, False)
    assert a3.tobytes() == a2.tobytes() and np.array_equal(c3, c2) and m3.tobytes() == mom.tobytes()
    # nothing selected: nothing changes; everything selected: the history call
    none = np.zeros((h, w), bool)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(R.refine(acc, cnt, mom, new, none, 8), (acc, cnt, mom)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(R.refine(acc, cnt, mom, new, ~none, 8), (wa, wc, wm)))


def test_refine_until_settles_and_counts():
    h, w = 4, 5
    acc, cnt, mom = np.zeros((h, w, 4), F32), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    frame = np.full((h, w, 4), 0.5, F32)
    # constant frames: every pixel has variance 0 once it has min_history frames, so the chain settles after them
    out = R.refine_until(acc, cnt, mom, lambda k: frame, 32, 10, None, (3, 1 << 24, 1, 0.05, 0.01))
    assert out[3:6] == (3, 3 * h * w, True) and out[6] == [h * w] * 3 and (out[1] == 3).all()
    out = R.refine_until(acc, cnt, mom, lambda k: frame, 32, 2, None, (3, 1 << 24, 1, 0.05, 0.01))
    assert out[3:6] == (2, 2 * h * w, False)
    out = R.refine_until(acc, cnt, mom, lambda k: frame, 32, 0, None)
    assert out[3:6] == (0, 0, False)


# ---- the defaults on oracle frames -------------------------------------------------------------------------------
def test_the_defaults_hold_conditions_a_b_c_against_the_uniform_curve():
    import refine_grid as G
    npix = G.SIZE[0] * G.SIZE[1]
    s_mse, s_pf, _ = G.adaptive("spheres", 64, R.DEFAULTS)
    s_uni = G.uniform_mse("spheres", -(-s_pf // npix))
    print(f"spheres, 64 passes: MSE {s_mse:.4f} at {s_pf / npix:.1f} equivalent frames; uniform {s_uni:.4f} at "
          f"{-(-s_pf // npix)} frames, {G.uniform_mse('spheres', 64):.4f} at 64")
    assert s_mse < s_uni  # (a)
    assert s_pf <= 32 * npix  # (b)
    b_mse, b_pf, counts = G.adaptive("box", 32, R.DEFAULTS)
    b_uni = G.uniform_mse("box", b_pf // npix)
    print(f"box, 32 passes: MSE {b_mse:.4f} at {b_pf / npix:.1f} equivalent frames, {counts[31] / npix:.3f} selected by "
          f"the 32nd pass; uniform {b_uni:.4f} at {b_pf // npix} frames")
    assert len(counts) == 32 and counts[31] >= 0.85 * npix and b_mse <= 1.1 * b_uni  # (c)
    # the own-pixel rule starves box (the reason the rule pools): it fails (c)
    r0 = R.DEFAULTS[:2] + (0,) + R.DEFAULTS[3:]
    _, _, c0 = G.adaptive("box", 32, r0)
    assert c0[31] < 0.85 * npix
