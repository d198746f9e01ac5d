"""Temporal upsampling on the CPU: the HIP-free coordinate header the resolve kernel shares
(epq_raytracer_amd/csrc/hrt_resolve_map.h), compiled into a stand-alone program (tests/cpp/resolve_map_test.cpp,
-ffp-contract=off; once more under AddressSanitizer and UBSan), against the numpy restatement tests/resolve_ref.py
word for word; then properties of the restatement itself, hrt_history_phase's coverage among them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import resolve_ref as R
from epq_raytracer_amd import _lib
from image_ref import same_floats

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
F32 = np.float32
N = 48
# the sizes the rates and the quality grid are measured at, both axes, and the largest widths
EXTRA = [(960, 1920), (540, 1080), (1920, 3840), (1080, 2160), (64, 128), (64, 160), (4096, 16384), (16384, 1),
         (1000, 16383), (1 << 24, 7)]
FIXED = (-0.5, -0.25, 0.0, 0.25, 0.5)


def build(target):
    subprocess.run(["make", "-s", "-C", CPP, "-f", "resolve_demo.mk", target], check=True)
    return os.path.join(CPP, target)


def expected_words(pairs):
    """The program's output for (ws, wt) pairs, from the restatement."""
    out = []
    for ws, wt in pairs:
        nx = R.phases(ws, wt)
        offs = [R.phase_offset(a, nx) for a in range(nx)]
        out.append(np.array([nx] + [o.view(np.uint32) for o in offs], np.uint32))
        for off in [F32(o) for o in FIXED] + offs:
            u, i, d, inside, own, ic = R.axis_map(wt, ws, off)
            rec = np.zeros((wt, 6), np.uint32)
            rec[:, 0], rec[:, 1], rec[:, 2] = u.view(np.uint32), i.view(np.uint32), d.view(np.uint32)
            rec[:, 3], rec[:, 4], rec[:, 5] = inside, own, ic.view(np.uint32)
            out.append(rec.reshape(-1))
    return np.concatenate(out)


@pytest.mark.parametrize("target", ["resolve_map_test", "resolve_map_test_san"])
def test_header_matches_the_restatement_bit_for_bit(target):
    """Every (Ws, W) in 1..48 x 1..48 and every x, the offsets -0.5, -0.25, 0, 0.25, 0.5 and every phase: u, i, d, the
    inside and acceptance tests, the clamp, and the phases' count and offsets; plus the sizes measured."""
    args = [str(N)] + [str(v) for p in EXTRA for v in p]
    r = subprocess.run([build(target)] + args, capture_output=True, timeout=600)
    assert r.returncode == 0 and b"ERROR" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:]
    got = np.frombuffer(r.stdout, np.uint32)
    want = expected_words([(ws, wt) for ws in range(1, N + 1) for wt in range(1, N + 1)] + EXTRA)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[0], got[bad[0][0]], want[bad[0][0]])


def test_library_history_phase_matches_the_restatement():
    lib = _lib.load()
    ox, oy = ctypes.c_float(), ctypes.c_float()
    for ws, w, hs, h in [(960, 1920, 540, 1080), (5, 13, 3, 7), (16, 8, 16, 8), (7, 7, 3, 3), (1, 3, 1, 2), (64, 160, 64, 128)]:
        n = R.phases(ws, w) * R.phases(hs, h)
        for k in list(range(2 * n + 1)) + [0xFFFFFFFF]:
            lib.hrt_history_phase(ws, w, hs, h, k, ctypes.byref(ox), ctypes.byref(oy))
            want = R.history_phase(ws, w, hs, h, k)
            assert (F32(ox.value).view(np.uint32), F32(oy.value).view(np.uint32)) == \
                   (want[0].view(np.uint32), want[1].view(np.uint32)), (ws, w, hs, h, k)
    lib.hrt_history_phase(4, 8, 4, 8, 3, None, None)  # NULL outputs are skipped
    info = _lib.ResolveInfo()
    lib.hrt_resolve_defaults(ctypes.byref(info))
    assert (info.offset_x, info.offset_y, info.max_history, info.flags) == (0.0, 0.0, R.DEFAULT_MAX_HISTORY, R.FILL)


# ---- properties of the restatement ------------------------------------------------------------------------------

def test_every_pixel_is_accepted_once_in_any_run_of_all_phases():
    """Over the nx phases of an axis (any nx consecutive k visit each once) every target index is accepted at least
    once, in float32 as specified: every Ws in 1..139 and W in 1..299."""
    for ws in range(1, 140):
        for w in range(1, 300):
            nx = R.phases(ws, w)
            offs = np.array([R.phase_offset(a, nx) for a in range(nx)], F32)
            seen = R.accepted_axis(w, ws, offs).any(axis=0)
            assert seen.all(), (ws, w, np.flatnonzero(~seen)[:4])


@pytest.mark.parametrize("size", [(960, 1920), (540, 1080), (1920, 3840), (1080, 2160), (64, 160), (1000, 16383)])
def test_the_sizes_measured_are_covered(size):
    ws, w = size
    nx = R.phases(ws, w)
    seen = np.zeros(w, bool)
    for a in range(nx):
        seen |= R.accepted_axis(w, ws, R.phase_offset(a, nx))
    assert seen.all()


def test_phases_of_equal_sizes_and_of_downscaling():
    for ws, w in [(7, 7), (16, 8), (9, 1), (1, 1)]:
        assert R.phases(ws, w) == 1 and R.phase_offset(0, 1) == 0
    assert R.phases(5, 13) == 3 and R.phases(5, 10) == 2 and R.phases(0, 4) == 1
    ks = [R.history_phase(5, 10, 3, 9, k) for k in range(12)]
    assert len(set(ks[:6])) == 6 and ks[:6] == ks[6:]  # raster order over nx * ny = 2 * 3 phases, then again


def image(h, w, seed, dtype=F32):
    rng = np.random.default_rng([seed, w, h])
    if dtype == np.uint8:
        img = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        img[..., 3] = 255
        return img
    img = (rng.uniform(0, 1, (h, w, 4)) ** 2 * 4).astype(F32)
    img[..., 3] = 1
    return img


@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_equal_sizes_with_offset_zero_are_accumulate_history(dtype):
    import history_ref as H
    import variance_ref as V
    h, w = 9, 13
    acc, new = image(h, w, 1, dtype), image(h, w, 2, dtype)
    cnt = np.random.default_rng(5).integers(0, 6, (h, w)).astype(np.uint32)
    mom = np.random.default_rng(6).uniform(0, 1, (h, w, 2)).astype(F32)
    out, ncnt, nmom, accepted, filled = R.resolve(acc, cnt, mom, new, max_history=4, flags=R.MOMENTS)
    assert accepted.all() and not filled.any()
    a2, c2, m2 = V.accumulate_history_moments(acc, cnt, mom, new, 4)
    assert np.array_equal(out.view(np.uint8), a2.view(np.uint8)) and np.array_equal(ncnt, c2)
    assert same_floats(nmom, m2).all()
    out, ncnt, nmom, _, _ = R.resolve(acc, cnt, mom, new, max_history=4, flags=0)
    a2, c2 = H.accumulate_history(acc, cnt, new, 4)
    assert np.array_equal(out.view(np.uint8), a2.view(np.uint8)) and np.array_equal(ncnt, c2) and nmom is mom


@pytest.mark.parametrize("ratio", [2, 4, 8, 3, 5, 6])
def test_an_integer_ratio_puts_each_accepted_sample_on_a_pixel_centre(ratio):
    """W = ratio * Ws with a phase offset: the accepted pixels are x = ratio * i + a, and each phase accepts every
    ratio-th pixel -- one of ratio disjoint classes.  With a power-of-two ratio the phase offsets are binary fractions
    and d == 0 exactly.  The offsets of any other ratio (1/3, 1/5, ...) are not binary32 numbers, so S20's own
    arithmetic leaves a rounding residue there (5.96e-8 and 2.38e-7 at Ws = 5, ratio 3): d is then held to the sum of
    its roundings -- half an ulp each for the quotient q, q - 0.5f and the final subtraction, 2^-24 for the offset's
    two operations -- which is at most 2^-24 (3 q + 1) <= 2^-22 (i + 1)."""
    for ws in (1, 5, 37, 64, 960):
        w = ws * ratio
        seen = np.zeros(w, int)
        for a in range(ratio):
            _, i, d, inside, own, _ = R.axis_map(w, ws, R.phase_offset(a, ratio))
            acc = inside & own
            if ratio & (ratio - 1) == 0:
                assert (d[acc] == 0).all()
            else:
                assert (d[acc].astype(np.float64) <= 2.0 ** -22 * (i[acc].astype(np.float64) + 1)).all()
            assert np.array_equal(np.flatnonzero(acc), np.arange(ws) * ratio + a)
            assert np.array_equal(i[acc], np.arange(ws, dtype=F32))
            seen += acc
        assert (seen == 1).all()


@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_fill_touches_only_pixels_without_history(dtype):
    hs, ws, h, w = 5, 7, 10, 14
    src, acc = image(hs, ws, 3, dtype), image(h, w, 4, dtype)
    cnt = np.random.default_rng(7).integers(0, 3, (h, w)).astype(np.uint32)
    off = R.history_phase(ws, w, hs, h, 1)
    out, ncnt, _, accepted, filled = R.resolve(acc, cnt, None, src, off, 8, R.FILL)
    assert accepted.sum() == hs * ws and filled.any()
    assert np.array_equal(filled, ~accepted & (cnt == 0))
    untouched = ~accepted & ~filled
    assert np.array_equal(out[untouched].view(np.uint8), acc[untouched].view(np.uint8))
    assert np.array_equal(ncnt[~accepted], cnt[~accepted])  # a fill leaves the count at 0
    # a filled pixel shows the source texel whose sample is nearest its centre (every value here is exact in binary32)
    ys, xs = np.nonzero(filled)
    sx = np.clip(np.floor((xs + 0.5) * ws / w - 0.5 - float(off[0]) + 0.5), 0, ws - 1).astype(int)
    sy = np.clip(np.floor((ys + 0.5) * hs / h - 0.5 - float(off[1]) + 0.5), 0, hs - 1).astype(int)
    assert np.array_equal(out[ys, xs, :3].view(np.uint8), src[sy, sx, :3].view(np.uint8))
    assert (out[ys, xs, 3] == (255 if dtype == np.uint8 else 1)).all()
    # ... and without FILL nothing but the accepted pixels changes
    out2, _, _, _, filled2 = R.resolve(acc, cnt, None, src, off, 8, 0)
    assert not filled2.any() and np.array_equal(out2[~accepted].view(np.uint8), acc[~accepted].view(np.uint8))
    assert np.array_equal(out2[accepted].view(np.uint8), out[accepted].view(np.uint8))


def test_guides_reject_pixels_of_another_surface():
    hs, ws, h, w = 4, 6, 8, 12
    src, acc = image(hs, ws, 8), image(h, w, 9)
    cnt = np.ones((h, w), np.uint32)
    lo, hi = np.zeros((hs, ws), _lib.HIT_DTYPE), np.zeros((h, w), _lib.HIT_DTYPE)
    lo["kind"], lo["index"] = 1, 3
    hi["kind"], hi["index"] = 1, 3
    hi["index"][2:5, 3:9] = 4  # a block of another sphere
    off = R.history_phase(ws, w, hs, h, 0)
    _, _, _, plain, _ = R.resolve(acc, cnt, None, src, off, 8, 0)
    out, ncnt, _, accepted, _ = R.resolve(acc, cnt, None, src, off, 8, 0, lo, hi)
    assert np.array_equal(accepted, plain & (hi["index"] == 3)) and accepted.sum() < plain.sum()
    assert np.array_equal(out[~accepted].view(np.uint8), acc[~accepted].view(np.uint8)) and (ncnt[~accepted] == 1).all()
