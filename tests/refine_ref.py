"""The adaptive refinement in numpy float32 (include/hip_raytrace.h hrt_refine_select, hrt_refine,
hrt_refine_until), written from the specification and independent of the kernels: tests/test_gpu_refine.py builds
every expected byte from it.  numpy's float32 arithmetic rounds every operation on its own (no contraction), its
division is IEEE's and a comparison with a NaN is false: each line below is one rounded operation of S17, in S17's
order."""
from __future__ import annotations

import numpy as np

import history_ref as H
import variance_ref as V
from denoise_ref import surface_keys

F32 = np.float32
# HRT_REFINE_MIN_HISTORY, HRT_REFINE_MAX_COUNT, HRT_REFINE_RADIUS, HRT_REFINE_TOLERANCE, HRT_REFINE_FLOOR
DEFAULTS = (4, 1 << 24, 1, 0.05, 0.01)


def select(cnt: np.ndarray, mom: np.ndarray, key=None, min_history=DEFAULTS[0], max_count=DEFAULTS[1], radius=DEFAULTS[2],
           tolerance=DEFAULTS[3], luminance_floor=DEFAULTS[4]) -> np.ndarray:
    """S17's selection: cnt (h, w) uint32, mom (h, w, 2) float32, key (h, w) uint32 surface keys or None (every key
    0).  Returns the (h, w) bool image of the selected pixels."""
    assert cnt.dtype == np.uint32 and mom.dtype == F32 and mom.shape == cnt.shape + (2,)
    assert 1 <= min_history <= max_count and 0 <= radius <= 3
    h, w = cnt.shape
    if key is None:
        key = np.zeros((h, w), np.uint32)
    tol, fl = F32(tolerance), F32(luminance_floor)
    tol2 = tol * tol
    with np.errstate(all="ignore"):
        m1, m2 = mom[..., 0], mom[..., 1]
        d = m2 - m1 * m1
        tv = np.where(d > 0, d, F32(0))
        se = tv / cnt.astype(F32)  # (used only where the tap is kept: N(q) >= min_history >= 1)
        usable = cnt >= np.uint32(min_history)
        pv, pm, k = np.zeros((h, w), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                ok, qy, qx = V._inside(h, w, dy, dx)
                ok &= key[qy, qx] == key
                ok &= usable[qy, qx]
                pv = np.where(ok, pv + se[qy, qx], pv)
                pm = np.where(ok, pm + m1[qy, qx], pm)
                k = np.where(ok, k + F32(1), k)
        a, b = pv / k, pm / k
        mu = np.where(b > fl, b, fl)
        crit = a > tol2 * (mu * mu)
    return np.where(cnt >= np.uint32(max_count), False, np.where(~usable, True, crit))


def select_scalar_radius0(cnt, mom, min_history, max_count, tolerance, luminance_floor) -> np.ndarray:
    """The own-pixel form of the rule (radius 0), pixel by pixel with scalar float32 operations."""
    h, w = cnt.shape
    out = np.zeros((h, w), bool)
    tol, fl = F32(tolerance), F32(luminance_floor)
    tol2 = tol * tol
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                n = int(cnt[y, x])
                if n >= max_count:
                    continue
                if n < min_history:
                    out[y, x] = True
                    continue
                m1, m2 = mom[y, x]
                d = m2 - m1 * m1
                tv = d if d > 0 else F32(0)
                a = (F32(0) + tv / F32(n)) / F32(1)
                b = (F32(0) + m1) / F32(1)
                mu = b if b > fl else fl
                out[y, x] = bool(a > tol2 * (mu * mu))
    return out


def pack_mask(sel: np.ndarray) -> np.ndarray:
    """The mask words of an (h, w) bool image: pixel i = x + y w is bit i & 31 of word i >> 5."""
    flat = np.ascontiguousarray(sel, bool).reshape(-1)
    words = (flat.size + 31) // 32
    bits = np.zeros(words * 32, np.uint8)
    bits[:flat.size] = flat
    return np.packbits(bits.reshape(words, 32), axis=1, bitorder="little").view("<u4").reshape(words).copy()


def unpack_mask(words: np.ndarray, shape) -> np.ndarray:
    """The (h, w) bool image of a mask; bits beyond the image are ignored."""
    h, w = shape
    bits = np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")
    return bits[:h * w].astype(bool).reshape(h, w)


def refine(acc, cnt, mom, frame, sel, max_history: int, moments: bool = True):
    """hrt_refine: the selected pixels of (acc, cnt, mom) take hrt_accumulate_history[_moments] of `frame`, the trace
    image of the pass's push block in the context's mode; every other pixel keeps its bytes.  (acc', cnt', mom')."""
    a2, c2 = H.accumulate_history(acc, cnt, frame, max_history)
    acc2, cnt2, mom2 = acc.copy(), cnt.copy(), mom.copy()
    acc2[sel], cnt2[sel] = a2[sel], c2[sel]
    if moments:
        mom2[sel] = V.fold_moments(cnt, mom, frame)[sel]
    return acc2, cnt2, mom2


def refine_until(acc, cnt, mom, frames, max_history: int, max_passes: int, key=None, rule=DEFAULTS):
    """hrt_refine_until: frames(k) = the trace image of pass k (rng_offset + k).  Returns (acc, cnt, mom, passes,
    pixel_frames, settled, selected per pass)."""
    passes, pixel_frames, settled, counts = 0, 0, False, []
    for k in range(max_passes):
        sel = select(cnt, mom, key, *rule)
        n = int(sel.sum())
        if n == 0:
            settled = True
            break
        acc, cnt, mom = refine(acc, cnt, mom, frames(k), sel, max_history, True)
        passes, pixel_frames = k + 1, pixel_frames + n
        counts.append(n)
    return acc, cnt, mom, passes, pixel_frames, settled, counts


def keys_of(hits, shape) -> np.ndarray:
    """S14's surface keys of width x height hrt_hit records."""
    return surface_keys(hits.reshape(shape))
