"""Object motion in the temporal history in numpy float32 (include/hip_raytrace.h
hrt_reproject_motion[_moments], include/hrt_host.h hrt_host_motion_between), written from the specification and
independent of the kernels: tests/test_gpu_motion.py builds every expected byte from it.  S21 is S15 with the moving
pixel's point taken through its object's G before step 4's subtraction and its normal through G's linear part before
step 8; the shared spellings (dot, cross, the view's fields) come from history_ref.py, steps 8 to 11 are restated here
with the normal as an argument.  Each line is one rounded binary32 operation, in the specification's order."""
from __future__ import annotations

import numpy as np

import history_ref as H
from denoise_ref import source_colour, surface_keys
from history_ref import BILINEAR, NEAREST, cross, dot, view_fields
from image_ref import unorm8

F32 = np.float32
MOVING = 1
MAX_OBJECTS = 65536
MOTION = np.dtype([("m", "<f4", (12,)), ("flags", "<u4"), ("reserved", "<u4", (3,))])  # hrt_motion
assert MOTION.itemsize == 64


def table(entries) -> np.ndarray:
    """An hrt_motion array of (m[12], flags) pairs."""
    out = np.zeros(len(entries), MOTION)
    for i, (m, flags) in enumerate(entries):
        out["m"][i] = np.asarray(m, F32)
        out["flags"][i] = flags
    return out


def static(n: int) -> np.ndarray:
    return np.zeros(n, MOTION)


def motion_between(prev_pose, cur_pose):
    """hrt_host_motion_between of two column-major 3x4 poses: (m[12] float32, flags)."""
    p, c = np.asarray(prev_pose, F32).reshape(12), np.asarray(cur_pose, F32).reshape(12)
    g = np.zeros(12, F32)
    with np.errstate(all="ignore"):
        for col in range(3):
            for r in range(3):
                g[3 * col + r] = (p[r] * c[col] + p[3 + r] * c[3 + col]) + p[6 + r] * c[6 + col]
        for r in range(3):
            lt = (g[r] * c[9] + g[3 + r] * c[10]) + g[6 + r] * c[11]
            g[9 + r] = p[9 + r] - lt
    return g, (0 if p.tobytes() == c.tobytes() else MOVING)


def entries_of(cur_hits: np.ndarray, spheres, meshes):
    """Per pixel of the (h, w) records: (moving, G) -- G (h, w, 12) float32, meaningful where moving."""
    kind = cur_hits["kind"].astype(np.uint32)
    kc = surface_keys(cur_hits)
    moving = np.zeros(cur_hits.shape, bool)
    g = np.zeros(cur_hits.shape + (12,), F32)
    for k, field, tab in ((1, "index", spheres), (2, "mesh", meshes)):
        if tab is None or len(tab) == 0:
            continue
        idx = cur_hits[field].astype(np.int64)
        sel = (kc != 0) & (kind == k) & (idx < len(tab))
        safe = np.where(sel, idx, 0)
        mv = sel & (tab["flags"][safe] != 0)
        moving |= mv
        g[mv] = tab["m"][safe[mv]]
    return moving, g


def source_coords(prev, cur, cur_hits: np.ndarray, moving: np.ndarray, g: np.ndarray):
    """S21 steps 1-7 for every pixel: (u, w, ok, te, kc) as history_ref.source_coords returns them."""
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
    p = [oc[k] + dn[k] * t for k in range(3)]
    pm = [((g[..., k] * p[0] + g[..., 3 + k] * p[1]) + g[..., 6 + k] * p[2]) + g[..., 9 + k] for k in range(3)]
    p = [np.where(moving, pm[k], p[k]) for k in range(3)]
    v = [np.where(hit, p[k] - op[k], dn[k]) for k in range(3)]
    q = [dot((mp[4 * j], mp[4 * j + 1], mp[4 * j + 2]), v) for j in range(3)]
    n = cross(dxp, dyp)
    s = dot(fp, n) / dot(q, n)
    r = [q[k] * s - fp[k] for k in range(3)]
    u = dot(r, dxp) / dot(dxp, dxp)
    wv = dot(r, dyp) / dot(dyp, dyp)
    te = np.sqrt(dot(v, v))
    return u, wv, s > 0, te, kc


def reproject(acc: np.ndarray, cnt: np.ndarray, prev, prev_hits: np.ndarray, cur, cur_hits: np.ndarray, spheres=None,
              meshes=None, filt: int = BILINEAR, depth_tolerance: float = H.DEFAULTS[0],
              min_normal_dot: float = H.DEFAULTS[1]):
    """hrt_reproject_motion: (acc', cnt'); spheres / meshes are hrt_motion arrays (MOTION) or None."""
    h, w = cnt.shape
    prev_hits, cur_hits = prev_hits.reshape(h, w), cur_hits.reshape(h, w)
    rgba8 = acc.dtype == np.uint8
    tol, mind = F32(depth_tolerance), F32(min_normal_dot)
    with np.errstate(all="ignore"):
        moving, g = entries_of(cur_hits, spheres, meshes)
        u, wv, ok, te, kc = source_coords(prev, cur, cur_hits, moving, g)
        kp = surface_keys(prev_hits)
        tp = np.ascontiguousarray(prev_hits["t"], F32)
        nc = [np.ascontiguousarray(cur_hits["normal"][..., k], F32) for k in range(3)]
        nm = [(g[..., k] * nc[0] + g[..., 3 + k] * nc[1]) + g[..., 6 + k] * nc[2] for k in range(3)]
        nc = [np.where(moving, nm[k], nc[k]) for k in range(3)]
        tol_te = tol * te

        def accepted(jx, jy, inside):
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


def reproject_moments(acc, cnt, mom, prev, prev_hits, cur, cur_hits, spheres=None, meshes=None, filt=BILINEAR,
                      depth_tolerance=H.DEFAULTS[0], min_normal_dot=H.DEFAULTS[1]):
    """hrt_reproject_motion_moments: (acc', cnt', mom') -- M travels as S16 says: as the r and g of a float image."""
    args = (prev, prev_hits, cur, cur_hits, spheres, meshes, filt, depth_tolerance, min_normal_dot)
    acc2, cnt2 = reproject(acc, cnt, *args)
    m4 = np.zeros(cnt.shape + (4,), F32)
    m4[..., :2] = mom
    mom2, cnt3 = reproject(m4, cnt, *args)
    assert np.array_equal(cnt2, cnt3)
    return acc2, cnt2, np.ascontiguousarray(mom2[..., :2])
