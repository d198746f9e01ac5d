"""The denoise pass in numpy float32 (include/hip_raytrace.h hrt_denoise), written from the
specification and independent of the kernels: tests/test_gpu_denoise.py builds every expected byte from it.
numpy's float32 arithmetic rounds every operation on its own (no contraction) and its division is IEEE's, so
each line below is one rounded operation of S14, in S14's order."""
from __future__ import annotations

import numpy as np

from image_ref import unorm8, unorm8_to_float

F32 = np.float32
K = (F32(0.375), F32(0.25), F32(0.0625))
DEFAULT_SIGMAS = (8.0, 0.25, 0.5)  # HRT_DENOISE_SIGMA_COLOUR / _NORMAL / _DEPTH


def surface_keys(hits: np.ndarray) -> np.ndarray:
    """S14's surface key of hrt_hit records (any shape): a sphere's index, a triangle's mesh, 0 for a miss."""
    kind, index, mesh = (hits[f].astype(np.uint32) for f in ("kind", "index", "mesh"))
    sphere = np.uint32(0x80000000) | (index & np.uint32(0x7FFFFFFF))
    tri = (mesh + np.uint32(1)) & np.uint32(0x7FFFFFFF)
    return np.where(kind == 1, sphere, np.where(kind == 2, tri, np.uint32(0))).astype(np.uint32)


def source_colour(img: np.ndarray) -> np.ndarray:
    """C0: the rgb of an (h, w, 4) image as float32 -- a uint8 byte k is float(k) / 255.0f."""
    return unorm8_to_float(img[..., :3]) if img.dtype == np.uint8 else np.ascontiguousarray(img[..., :3], F32)


def one_pass(c: np.ndarray, i: int, sigmas, guide=None) -> np.ndarray:
    """S14's pass i on c (h, w, 3) float32; guide = (normal (h, w, 3), t (h, w), key (h, w)) or None."""
    h, w = c.shape[:2]
    s = 1 << i
    sc, sn, sd = (F32(v) for v in sigmas)
    kc = F32(np.ldexp(F32(1) / (sc * sc), 2 * i))
    acc, wsum = np.zeros((h, w, 3), F32), np.zeros((h, w), F32)
    if guide is not None:
        n, t, key = guide
        kn = F32(1) / sn
        kd = F32(1) / ((sd * t) * F32(s))
    ys, xs = np.mgrid[0:h, 0:w]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qy, qx = ys + s * dy, xs + s * dx
            ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            cq = c[qy, qx]
            e = c - cq
            dc = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            wc = F32(1) / (F32(1) + dc * kc)
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
            # a skipped tap adds nothing: its sums are left as they are (not "+ 0", which would turn -0 or NaN)
            acc = np.where(ok[..., None], acc + wgt[..., None] * cq, acc)
            wsum = np.where(ok, wsum + wgt, wsum)
    return (acc / wsum[..., None]).astype(F32)


def denoise(img: np.ndarray, iterations: int, sigmas=DEFAULT_SIGMAS, hits=None, fmt_rgba8: bool = False) -> np.ndarray:
    """hrt_denoise of an (h, w, 4) uint8 or float32 image; hits: (h, w) hrt_hit records or None.  Returns
    (h, w, 4) float32 with alpha 1.0, or with fmt_rgba8 the uint8 image S7's store makes of it (alpha 255)."""
    c = source_colour(img)
    guide = None
    if hits is not None:
        hits = hits.reshape(c.shape[:2])
        guide = (np.ascontiguousarray(hits["normal"], F32), np.ascontiguousarray(hits["t"], F32), surface_keys(hits))
    with np.errstate(all="ignore"):
        for i in range(iterations):
            c = one_pass(c, i, sigmas, guide)
    out = np.ones(c.shape[:2] + (4,), F32)
    out[..., :3] = c
    return unorm8(out) if fmt_rgba8 else out
