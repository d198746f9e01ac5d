"""Guided upsampling in numpy float32 (include/hip_raytrace.h hrt_upsample), written from the
specification and independent of the kernel: tests/test_gpu_upsample.py builds every expected byte from it, and
tests/test_upsample_ref.py holds the shared coordinate header (epq_raytracer_amd/csrc/hrt_upsample_map.h) to it.
numpy's float32 arithmetic rounds every operation on its own (no contraction) and its division is IEEE's, so each
line below is one rounded operation of S19, in S19's order."""
from __future__ import annotations

import numpy as np

from denoise_ref import source_colour, surface_keys
from image_ref import unorm8

F32 = np.float32
DEFAULT_SIGMAS = (0.25, 0.5)  # HRT_DENOISE_SIGMA_NORMAL / _DEPTH (hrt_upsample_defaults)
DEFAULT_FOOTPRINT = 2         # HRT_UPSAMPLE_FOOTPRINT
TAPS = {2: (0, 1), 4: (-1, 0, 1, 2)}
INV_R = {2: F32(1.0), 4: F32(0.5)}


def coord(n_t: int, n_s: int) -> np.ndarray:
    """u of every target index along one axis: ((float(x) + 0.5f) * float(Ws)) / float(Wt) - 0.5f."""
    x = np.arange(n_t, dtype=np.uint32).astype(F32)
    return (((x + F32(0.5)) * F32(n_s)) / F32(n_t)) - F32(0.5)


def axis_taps(n_t: int, n_s: int, footprint: int):
    """One axis of S19: (u, x0, [(xj, inside, w) per tap offset, ascending]); every array has n_t entries.  inside
    is the float bounds test, w = 1.0f - fabsf(u - xj) * inv_r (computed for every tap, inside or not)."""
    u = coord(n_t, n_s)
    x0 = np.floor(u).astype(F32)
    taps = []
    for e in TAPS[footprint]:
        xj = x0 + F32(e)
        inside = (xj >= F32(0)) & (xj <= F32(n_s - 1))
        w = F32(1) - np.abs(u - xj) * INV_R[footprint]
        taps.append((xj, inside, w.astype(F32)))
    return u, x0, taps


def nearest(n_t: int, n_s: int) -> np.ndarray:
    """The fallback's texel per target index: ((2x+1) Ws) div (2 Wt) (Python ints: no overflow)."""
    return np.array([((2 * x + 1) * n_s) // (2 * n_t) for x in range(n_t)], dtype=np.int64)


def upsample(low: np.ndarray, low_hits: np.ndarray, high_hits: np.ndarray, footprint: int = DEFAULT_FOOTPRINT,
             sigmas=DEFAULT_SIGMAS, fmt_rgba8: bool = False, with_info: bool = False):
    """hrt_upsample of the (hs, ws, 3 or 4) low image -- uint8 or float32 texels, or a filter's float result --
    with low_hits (hs, ws) and high_hits (ht, wt) hrt_hit records.  Returns (ht, wt, 4) float32 with alpha 1.0, or
    with fmt_rgba8 the uint8 image S7's store makes of it (alpha 255); with_info also (kept, fallback): the number
    of taps each pixel kept (int, (ht, wt)) and whether its store took the nearest texel (bool)."""
    c = source_colour(low)
    hs, ws = c.shape[:2]
    ht, wt = high_hits.shape
    low_hits = low_hits.reshape(hs, ws)
    sn, sd = (F32(v) for v in sigmas)
    nq, tq, kq = (np.ascontiguousarray(low_hits["normal"], F32), np.ascontiguousarray(low_hits["t"], F32),
                  surface_keys(low_hits))
    n, tp, kp = (np.ascontiguousarray(high_hits["normal"], F32), np.ascontiguousarray(high_hits["t"], F32),
                 surface_keys(high_hits))
    with np.errstate(all="ignore"):
        kn = F32(1) / sn
        kd = F32(1) / (sd * tp)
        _, _, xt = axis_taps(wt, ws, footprint)
        _, _, yt = axis_taps(ht, hs, footprint)
        acc, wsum = np.zeros((ht, wt, 3), F32), np.zeros((ht, wt), F32)
        kept = np.zeros((ht, wt), np.int64)
        sky = kp == 0
        for yj, y_in, wy in yt:
            for xj, x_in, wx in xt:
                ok = (y_in & (wy > 0))[:, None] & (x_in & (wx > 0))[None, :]
                qy = np.where(y_in, yj, 0).astype(np.int64)[:, None]
                qx = np.where(x_in, xj, 0).astype(np.int64)[None, :]
                ok = ok & (kq[qy, qx] == kp)
                h = wx[None, :] * wy[:, None]
                g = nq[qy, qx]
                dot = (n[..., 0] * g[..., 0] + n[..., 1] * g[..., 1]) + n[..., 2] * g[..., 2]
                a = F32(1) - (F32(1) - dot) * kn
                b = F32(1) - np.abs(tp - tq[qy, qx]) * kd
                wn = np.where(sky, F32(1), np.where(a > 0, a, F32(0)))
                wd = np.where(sky, F32(1), np.where(b > 0, b, F32(0)))
                w = ((h * wn) * wd).astype(F32)
                cq = c[qy, qx]
                # a skipped tap adds nothing: its sums are left as they are (not "+ 0", which would turn -0 or NaN)
                acc = np.where(ok[..., None], acc + w[..., None] * cq, acc)
                wsum = np.where(ok, wsum + w, wsum)
                kept += ok
        fallback = ~(wsum > 0)
        near = c[nearest(ht, hs)[:, None], nearest(wt, ws)[None, :]]
        rgb = np.where(fallback[..., None], near, acc / wsum[..., None]).astype(F32)
    out = np.ones((ht, wt, 4), F32)
    out[..., :3] = rgb
    res = unorm8(out) if fmt_rgba8 else out
    return (res, kept, fallback) if with_info else res


def nearest_upsample(low: np.ndarray, wt: int, ht: int) -> np.ndarray:
    """What hrt_present's nearest rule makes of the low image at wt x ht, without the flip: (ht, wt, 3) float32."""
    c = source_colour(low)
    hs, ws = c.shape[:2]
    return c[nearest(ht, hs)[:, None], nearest(wt, ws)[None, :]]
