"""The temporal history in numpy float32 (include/hip_raytrace.h hrt_reproject,
hrt_accumulate_history), written from the specification and independent of the kernels:
tests/test_gpu_history.py builds every expected byte from it.  numpy's float32 arithmetic rounds every
operation on its own (no contraction), its division and square root are IEEE's, and a comparison with a NaN
is false: each line below is one rounded operation of S15, in S15's order."""
from __future__ import annotations

import numpy as np

import image_ref as I
from denoise_ref import source_colour, surface_keys
from image_ref import unorm8

F32 = np.float32
NEAREST, BILINEAR = 0, 1
DEFAULTS = (0.02, 0.9)  # HRT_REPROJECT_DEPTH_TOLERANCE / _MIN_NORMAL_DOT


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def view_fields(view):
    """(cam_pos[3], M[16], first[3], dx[3], dy[3]) of anything with hrt_view's fields, as float32 scalars."""
    def f(name, n):
        return [F32(v) for v in list(getattr(view, name))[:n]]
    return f("cam_pos", 3), f("cam_alignment_mat", 16), f("grid_first", 3), f("grid_dx", 3), f("grid_dy", 3)


def accumulate_history(acc: np.ndarray, cnt: np.ndarray, new: np.ndarray, max_history: int):
    """hrt_accumulate_history on (h, w, 4) uint8 or float32 images and (h, w) uint32 counts: (acc', cnt')."""
    assert acc.dtype == new.dtype and acc.shape == new.shape and cnt.shape == acc.shape[:2] and cnt.dtype == np.uint32
    fold = I.fold_rgba8 if acc.dtype == np.uint8 else I.fold_rgba32f
    out = np.empty_like(acc)
    for n in np.unique(cnt):
        m = cnt == n
        if n == 0:
            first = new[m].copy()
            first[..., 3] = 255 if acc.dtype == np.uint8 else 1.0
            out[m] = first
        else:
            out[m] = fold(int(n), acc[m], new[m])
    nxt = np.minimum(cnt.astype(np.int64) + 1, int(max_history)).astype(np.uint32)
    return out, nxt


def source_coords(prev, cur, cur_hits: np.ndarray):
    """S15 steps 1-7 for every pixel of the (h, w) records cur_hits: (u, w, ok, te, kc) with ok = s > 0."""
    h, w = cur_hits.shape
    oc, mc, fc, dxc, dyc = view_fields(cur)
    op, mp, fp, dxp, dyp = view_fields(prev)
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs.astype(F32), ys.astype(F32)
    c = [(fc[k] + dxc[k] * fx) + dyc[k] * fy for k in range(3)]
    d = [(mc[k] * c[0] + mc[4 + k] * c[1]) + mc[8 + k] * c[2] for k in range(3)]
    ln = np.sqrt(dot(d, d))
    dn = [d[k] / ln for k in range(3)]
    kc = surface_keys(cur_hits)
    t = np.ascontiguousarray(cur_hits["t"], F32)
    hit = kc != 0
    v = [np.where(hit, (oc[k] + dn[k] * t) - op[k], dn[k]) for k in range(3)]
    q = [dot((mp[4 * j], mp[4 * j + 1], mp[4 * j + 2]), v) for j in range(3)]
    n = cross(dxp, dyp)
    s = dot(fp, n) / dot(q, n)
    r = [q[k] * s - fp[k] for k in range(3)]
    u = dot(r, dxp) / dot(dxp, dxp)
    wv = dot(r, dyp) / dot(dyp, dyp)
    te = np.sqrt(dot(v, v))
    return u, wv, s > 0, te, kc


def reproject(acc: np.ndarray, cnt: np.ndarray, prev, prev_hits: np.ndarray, cur, cur_hits: np.ndarray,
              filt: int = BILINEAR, depth_tolerance: float = DEFAULTS[0], min_normal_dot: float = DEFAULTS[1]):
    """hrt_reproject: (acc', cnt') of an (h, w, 4) uint8 or float32 accumulator and its (h, w) uint32 counts;
    the hit arrays are (h, w) hrt_hit records."""
    h, w = cnt.shape
    prev_hits, cur_hits = prev_hits.reshape(h, w), cur_hits.reshape(h, w)
    rgba8 = acc.dtype == np.uint8
    tol, mind = F32(depth_tolerance), F32(min_normal_dot)
    with np.errstate(all="ignore"):
        u, wv, ok, te, kc = source_coords(prev, cur, cur_hits)
        kp = surface_keys(prev_hits)
        tp = np.ascontiguousarray(prev_hits["t"], F32)
        nc = [np.ascontiguousarray(cur_hits["normal"][..., k], F32) for k in range(3)]
        tol_te = tol * te

        def accepted(jx, jy, inside):
            """Step 8 for the source pixels (jx, jy) (int64 arrays; anything where not `inside`)."""
            jx, jy = np.where(inside, jx, 0), np.where(inside, jy, 0)
            a = inside & (cnt[jy, jx] > 0) & (kp[jy, jx] == kc)
            npv = [prev_hits["normal"][jy, jx, k] for k in range(3)]
            geo = (np.abs(te - tp[jy, jx]) <= tol_te) & (dot(nc, npv) >= mind)
            return a & ((kc == 0) | geo), jx, jy

        def to_index(f, valid):
            return np.where(valid, f, F32(0)).astype(np.int64)

        out = np.zeros_like(acc)
        out[..., 3] = 255 if rgba8 else 1.0
        ncnt = np.zeros((h, w), np.uint32)
        if filt == NEAREST:
            ix, iy = np.floor(u + F32(0.5)), np.floor(wv + F32(0.5))
            inside = ok & (ix >= 0) & (ix <= F32(w - 1)) & (iy >= 0) & (iy <= F32(h - 1))
            a, jx, jy = accepted(to_index(ix, inside), to_index(iy, inside), inside)
            out[a] = acc[jy[a], jx[a]]
            ncnt[a] = cnt[jy[a], jx[a]]
            return out, ncnt
        assert filt == BILINEAR
        x0, y0 = np.floor(u), np.floor(wv)
        inside = ok & (x0 >= -1) & (x0 <= F32(w - 1)) & (y0 >= -1) & (y0 <= F32(h - 1))
        fa, fb = u - x0, wv - y0
        ix0, iy0 = to_index(x0, inside), to_index(y0, inside)
        c0 = source_colour(acc)
        sums = np.zeros((h, w, 3), F32)
        wsum = np.zeros((h, w), F32)
        nmin = np.full((h, w), 0xFFFFFFFF, np.uint32)
        used_any = np.zeros((h, w), bool)
        for ex, ey in ((0, 0), (1, 0), (0, 1), (1, 1)):
            wx = fa if ex else F32(1) - fa
            wy = fb if ey else F32(1) - fb
            wt = wx * wy
            jx, jy = ix0 + ex, iy0 + ey
            tap_in = inside & (jx >= 0) & (jx < w) & (jy >= 0) & (jy < h)
            a, jx, jy = accepted(jx, jy, tap_in)
            used = a & (wt > 0)
            # an unused tap adds nothing: the sums are left as they are
            sums = np.where(used[..., None], sums + wt[..., None] * c0[jy, jx], sums)
            wsum = np.where(used, wsum + wt, wsum)
            nmin = np.where(used, np.minimum(nmin, cnt[jy, jx]), nmin)
            used_any |= used
        res = sums / wsum[..., None]
        if rgba8:
            out[used_any, :3] = unorm8(res)[used_any]
        else:
            out[used_any, :3] = res[used_any]
        ncnt[used_any] = nmin[used_any]
        return out, ncnt
