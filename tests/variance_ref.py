"""The variance-guided denoise in numpy float32 (include/hip_raytrace.h hrt_denoise_variance,
hrt_accumulate_history_moments, hrt_reproject_moments), written from the specification and independent of the
kernels: tests/test_gpu_variance.py builds every expected byte from it.  numpy's float32 arithmetic rounds every
operation on its own (no contraction), its division is IEEE's and a comparison with a NaN is false: each line
below is one rounded operation of S16, in S16's order."""
from __future__ import annotations

import numpy as np

import history_ref as H
import image_ref as I
from denoise_ref import K, source_colour, surface_keys
from image_ref import unorm8

F32 = np.float32
G = (F32(0.5), F32(0.25))
LUM = (F32(0.2126), F32(0.7152), F32(0.0722))
# HRT_VARIANCE_SIGMA, HRT_VARIANCE_FLOOR, HRT_VARIANCE_MIN_HISTORY, HRT_DENOISE_SIGMA_NORMAL, HRT_DENOISE_SIGMA_DEPTH
DEFAULTS = (4.0, 1e-10, 4, 0.25, 0.5)


def lum(c: np.ndarray) -> np.ndarray:
    """S16's luminance of (..., 3) float32 colours."""
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def fold_moments(cnt: np.ndarray, mom: np.ndarray, new: np.ndarray) -> np.ndarray:
    """M after hrt_accumulate_history_moments: mom (h, w, 2) float32, cnt the counts before the update, new the
    trace image ((h, w, 4) uint8 or float32)."""
    assert mom.dtype == F32 and mom.shape == cnt.shape + (2,)
    with np.errstate(all="ignore"):
        l = lum(source_colour(new))
        sample = np.stack([l, l * l], -1)
        out = np.empty_like(mom)
        for n in np.unique(cnt):
            m = cnt == n
            if n == 0:
                out[m] = sample[m]
            else:
                _, ff, ff1 = I._denominators(int(n))
                out[m] = (sample[m] + mom[m] * ff) / ff1
    return out


def accumulate_history_moments(acc, cnt, mom, new, max_history: int):
    """hrt_accumulate_history_moments: (acc', cnt', mom')."""
    acc2, cnt2 = H.accumulate_history(acc, cnt, new, max_history)
    return acc2, cnt2, fold_moments(cnt, mom, new)


def reproject_moments(acc, cnt, mom, prev, prev_hits, cur, cur_hits, filt=H.BILINEAR, depth_tolerance=H.DEFAULTS[0],
                      min_normal_dot=H.DEFAULTS[1]):
    """hrt_reproject_moments: (acc', cnt', mom').  M is carried as two colour channels of an RGBA32F texel are by
    S15's steps 8-11, so it goes through S15's restatement as the r and g of a float image."""
    acc2, cnt2 = H.reproject(acc, cnt, prev, prev_hits, cur, cur_hits, filt, depth_tolerance, min_normal_dot)
    m4 = np.zeros(cnt.shape + (4,), F32)
    m4[..., :2] = mom
    mom2, cnt3 = H.reproject(m4, cnt, prev, prev_hits, cur, cur_hits, filt, depth_tolerance, min_normal_dot)
    assert np.array_equal(cnt2, cnt3)
    return acc2, cnt2, np.ascontiguousarray(mom2[..., :2])


def _inside(h, w, dy, dx):
    ys, xs = np.mgrid[0:h, 0:w]
    qy, qx = ys + dy, xs + dx
    ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
    return ok, np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)


def variance_estimate(c0: np.ndarray, cnt: np.ndarray, mom: np.ndarray, key: np.ndarray, min_history: int) -> np.ndarray:
    """V0 of S16: temporal where cnt >= min_history, else the 7 x 7 spatial estimate over taps of the same key."""
    h, w = cnt.shape
    with np.errstate(all="ignore"):
        m1, m2 = mom[..., 0], mom[..., 1]
        d = m2 - m1 * m1
        tv = np.where(d > 0, d, F32(0))
        temporal = tv / cnt.astype(F32)
        lq_all = lum(c0)
        s1, s2, k = np.zeros((h, w), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                ok, qy, qx = _inside(h, w, dy, dx)
                ok &= key[qy, qx] == key
                lq = lq_all[qy, qx]
                s1 = np.where(ok, s1 + lq, s1)
                s2 = np.where(ok, s2 + lq * lq, s2)
                k = np.where(ok, k + F32(1), k)
        mean = s1 / k
        e = s2 / k - mean * mean
        spatial = np.where(e > 0, e, F32(0))
    return np.where(cnt >= np.uint32(min_history), temporal, spatial).astype(F32)


def prefilter(v: np.ndarray) -> np.ndarray:
    """vg of S16: the 3 x 3 Gaussian of the variance image, taps one pixel apart, renormalised at the border."""
    h, w = v.shape
    va, gs = np.zeros((h, w), F32), np.zeros((h, w), F32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            ok, qy, qx = _inside(h, w, dy, dx)
            g = G[abs(dx)] * G[abs(dy)]
            va = np.where(ok, va + g * v[qy, qx], va)
            gs = np.where(ok, gs + g, gs)
    return va / gs


def one_pass(c: np.ndarray, v: np.ndarray, i: int, sigma_variance, variance_floor, sigma_normal, sigma_depth, guide=None):
    """S16's pass i on colours c (h, w, 3) and variances v (h, w); guide = (normal, t, key) or None: (c', v')."""
    h, w = v.shape
    s = 1 << i
    sv, fl, sn, sd = (F32(x) for x in (sigma_variance, variance_floor, sigma_normal, sigma_depth))
    sv2 = sv * sv
    kv = F32(1) / ((sv2 * prefilter(v)) + fl)
    acc, vacc, wsum = np.zeros((h, w, 3), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
    if guide is not None:
        n, t, key = guide
        kn = F32(1) / sn
        kd = F32(1) / ((sd * t) * F32(s))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ok, qy, qx = _inside(h, w, s * dy, s * dx)
            cq = c[qy, qx]
            e = c - cq
            dc = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            wc = F32(1) / (F32(1) + dc * kv)
            wgt = (K[abs(dx)] * K[abs(dy)]) * wc
            if guide is not None:
                ok &= key[qy, qx] == key
                nq = n[qy, qx]
                dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                a = F32(1) - (F32(1) - dot) * kn
                b = F32(1) - np.abs(t - t[qy, qx]) * kd
                flat = key == 0
                wn = np.where(flat, F32(1), np.where(a > 0, a, F32(0)))
                wd = np.where(flat, F32(1), np.where(b > 0, b, F32(0)))
                wgt = (wgt * wn) * wd
            # a skipped tap adds nothing: its sums are left as they are
            acc = np.where(ok[..., None], acc + wgt[..., None] * cq, acc)
            vacc = np.where(ok, vacc + (wgt * wgt) * v[qy, qx], vacc)
            wsum = np.where(ok, wsum + wgt, wsum)
    return (acc / wsum[..., None]).astype(F32), (vacc / (wsum * wsum)).astype(F32)


def denoise_variance(acc: np.ndarray, cnt: np.ndarray, mom: np.ndarray, iterations: int, params=DEFAULTS, hits=None,
                     fmt_rgba8: bool = False):
    """hrt_denoise_variance of an (h, w, 4) uint8 or float32 accumulator with its counts and moments; params =
    (sigma_variance, variance_floor, min_history, sigma_normal, sigma_depth); hits: (h, w) hrt_hit records or None.
    Returns (image, variance): (h, w, 4) float32 with alpha 1.0 (with fmt_rgba8 the uint8 image S7's store makes of
    it, alpha 255) and the (h, w) float32 V_iterations."""
    sv, fl, min_history, sn, sd = params
    c = source_colour(acc)
    h, w = c.shape[:2]
    guide = None
    key = np.zeros((h, w), np.uint32)
    if hits is not None:
        hits = hits.reshape(h, w)
        key = surface_keys(hits)
        guide = (np.ascontiguousarray(hits["normal"], F32), np.ascontiguousarray(hits["t"], F32), key)
    with np.errstate(all="ignore"):
        v = variance_estimate(c, cnt, mom, key, min_history)
        for i in range(iterations):
            c, v = one_pass(c, v, i, sv, fl, sn, sd, guide)
    out = np.ones((h, w, 4), F32)
    out[..., :3] = c
    return (unorm8(out) if fmt_rgba8 else out), v
