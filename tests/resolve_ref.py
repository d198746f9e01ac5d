"""The fold across resolutions in numpy float32 (include/hip_raytrace.h
hrt_accumulate_history_from, hrt_history_phase), written from the specification and independent of the kernel:
tests/test_gpu_resolve.py builds every expected byte from it, and tests/test_resolve_ref.py holds the shared
coordinate header (epq_raytracer_amd/csrc/hrt_resolve_map.h) to it.  numpy's float32 arithmetic rounds every
operation on its own (no contraction) and its division is IEEE's, so each line below is one rounded operation of
S20, in S20's order.  An accepted pixel's step is history_ref's / variance_ref's, the restatement of
hrt_accumulate_history[_moments]."""
from __future__ import annotations

import numpy as np

import history_ref as H
import variance_ref as V
from denoise_ref import surface_keys
from upsample_ref import coord

F32 = np.float32
FILL, MOMENTS = 1, 2   # HRT_RESOLVE_FILL / HRT_RESOLVE_MOMENTS
DEFAULT_MAX_HISTORY = 32  # hrt_resolve_defaults


def phases(n_s: int, n_t: int) -> int:
    """nx = max(1, ceil(W / Ws)) in integers (a size of 0 counts as one phase)."""
    return max(1, -(-n_t // n_s)) if n_s else 1


def phase_offset(a: int, n: int) -> np.float32:
    """(float(a) + 0.5f) / float(n) - 0.5f."""
    return F32((F32(a) + F32(0.5)) / F32(n) - F32(0.5))


def history_phase(ws: int, w: int, hs: int, h: int, k: int):
    """hrt_history_phase: (ox, oy) of frame k."""
    nx, ny = phases(ws, w), phases(hs, h)
    return phase_offset(k % nx, nx), phase_offset((k // nx) % ny, ny)


def axis_map(n_t: int, n_s: int, offset):
    """One axis of S20 for every target index: (u, i, d, inside, own, ic) -- i, d and ic float32, ic the clamp of i
    to [0, n_s - 1]; own is the test d * float(W) <= 0.5f * float(Ws) alone (accepted needs inside too).  An array of
    offsets gives one row per offset."""
    u = (coord(n_t, n_s) - np.asarray(offset, F32)[..., None]).astype(F32)
    i = np.floor(u + F32(0.5)).astype(F32)
    d = np.abs(u - i).astype(F32)
    inside = (i >= F32(0)) & (i <= F32(n_s - 1))
    own = (d * F32(n_t)).astype(F32) <= F32(0.5) * F32(n_s)
    ic = np.minimum(np.maximum(i, F32(0)), F32(n_s - 1)).astype(F32)
    return u, i, d, inside, own, ic


def accepted_axis(n_t: int, n_s: int, offset) -> np.ndarray:
    """Whether each target index takes a sample along this axis (inside and own)."""
    _, _, _, inside, own, _ = axis_map(n_t, n_s, offset)
    return inside & own


def resolve(acc: np.ndarray, cnt: np.ndarray, mom, src: np.ndarray, offset=(0.0, 0.0),
            max_history: int = DEFAULT_MAX_HISTORY, flags: int = FILL, src_hits=None, hits=None):
    """hrt_accumulate_history_from.  acc (h, w, 4) uint8 or float32, cnt (h, w) uint32, mom (h, w, 2) float32 or None
    (needed with MOMENTS), src (hs, ws, 4) of acc's dtype; the hit arrays (hs, ws) and (h, w) hrt_hit records, both
    or neither.  Returns (acc', cnt', mom', accepted, filled): mom' is mom itself without MOMENTS; the last two are
    (h, w) bool."""
    h, w = cnt.shape
    hs, ws = src.shape[:2]
    assert acc.dtype == src.dtype and acc.shape == (h, w, 4) and cnt.dtype == np.uint32
    assert (src_hits is None) == (hits is None)
    with np.errstate(all="ignore"):
        _, _, _, x_in, x_own, xc = axis_map(w, ws, offset[0])
        _, _, _, y_in, y_own, yc = axis_map(h, hs, offset[1])
        accepted = (y_in & y_own)[:, None] & (x_in & x_own)[None, :]
        qy, qx = yc.astype(np.int64)[:, None], xc.astype(np.int64)[None, :]
        if hits is not None:
            ks = surface_keys(src_hits.reshape(hs, ws))
            kt = surface_keys(hits.reshape(h, w))
            accepted = accepted & (ks[qy, qx] == kt)
        tex = np.ascontiguousarray(src[qy, qx])  # T(ic, jc) per target pixel (T(i, j) where accepted)
        step_acc, step_cnt = H.accumulate_history(acc, cnt, tex, max_history)
        filled = ~accepted & (cnt == 0) if flags & FILL else np.zeros((h, w), bool)
        first = tex.copy()
        first[..., 3] = 255 if acc.dtype == np.uint8 else 1.0
        out = np.where(accepted[..., None], step_acc, np.where(filled[..., None], first, acc))
        ncnt = np.where(accepted, step_cnt, cnt).astype(np.uint32)
        nmom = mom
        if flags & MOMENTS:
            nmom = np.where(accepted[..., None], V.fold_moments(cnt, mom, tex), mom).astype(F32)
    return out, ncnt, nmom, accepted, filled
