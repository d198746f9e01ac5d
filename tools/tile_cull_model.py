#!/usr/bin/env python3
"""Numpy model of the primary tile lists: camera_lists' cull record, the cap rule
(tile_bundle + bundle_keep) and the corner-direction rule per tile and per pixel (build_tile_list,
refine_tile_list in epq_raytracer_amd/csrc/hrt_kernels.hip), for a preset and an image size.

Two arithmetics:
  float64 (default)  the rules as mathematics, for the table below and for reasoning about the bounds;
  float32 (--mirror) every operation in the kernel's order and precision (FMAs where hrt_math.h writes them,
                     separately rounded products and sums elsewhere), so the lists can be held against
                     hrt_debug_tile_lists entry for entry (tests/test_gpu_tile_cull.py).

Prints, per rule: tiles with a list (non-sky), list entries over all tiles, and the hit tiles the rule
misses (tiles where a float64 Moller-Trumbore test of the pixels' centre and jitter-box corner rays finds a
hit on a triangle the rule left out; must be 0).

    python tools/tile_cull_model.py island 1920 1080
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CAP = 64  # kTileCapVgpr
BORDER = 1e-4  # an entry is "borderline" when a compared value lies within this (relative) of its threshold


class Arith:
    """float64, or float32 with the kernel's rounding (fma = one rounding; a * b + c = two)."""

    def __init__(self, mirror: bool):
        self.T = np.float32 if mirror else np.float64
        self.mirror = mirror

    def a(self, v):
        return np.asarray(v, np.float32).astype(self.T)

    def fma(self, a, b, c):
        if not self.mirror:
            return a * b + c
        # the product of two float32 is exact in float64; one more rounding to float32 (a double rounding
        # only when the float64 sum lands on a float32 tie: never within BORDER of a threshold by chance)
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)

    def dot(self, a, b):  # hrt_math.h dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))
        return self.fma(a[..., 2], b[..., 2], self.fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))

    def cross(self, a, b):  # hrt_math.h cross
        return np.stack([self.fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])),
                         self.fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                         self.fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1)

    def normalize(self, a):  # hrt_math.h normalize: v / sqrt(dot(v, v)), every step correctly rounded
        return a / np.sqrt(self.dot(a, a))[..., None]

    def box_dir(self, M, v):  # hrt_kernels.hip box_dir (products and sums rounded separately)
        w = np.stack([(M[0] * v[..., 0] + M[4] * v[..., 1]) + M[8] * v[..., 2],
                      (M[1] * v[..., 0] + M[5] * v[..., 1]) + M[9] * v[..., 2],
                      (M[2] * v[..., 0] + M[6] * v[..., 1]) + M[10] * v[..., 2]], -1)
        return self.normalize(w)


def camera_records(ar: Arith, cam_pos, tris, meshes):
    """camera_lists: per mesh the triangles with num_t > 0 in buffer order -> (global index, mesh, C0..C4)."""
    T = ar.T
    o = ar.a(cam_pos[:3])
    idx, mesh_of = [], []
    for m, rec in enumerate(meshes):
        k = np.arange(int(rec["first_index"]), int(rec["first_index"]) + int(rec["len"]))
        idx.append(k)
        mesh_of.append(np.full(k.size, m))
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    mesh_of = np.concatenate(mesh_of) if mesh_of else np.zeros(0, np.int64)
    a, e1 = ar.a(tris["a"][idx, :3]), ar.a(tris["edge_one"][idx, :3])
    e2, n = ar.a(tris["edge_two"][idx, :3]), ar.a(tris["normal"][idx, :3])
    ao = o - a
    keep = ar.dot(ao, n) > 0
    idx, mesh_of, ao, e1, e2, n = idx[keep], mesh_of[keep], ao[keep], e1[keep], e2[keep], n[keep]
    gu, h = ar.cross(e2, ao), ar.cross(e1, ao)
    kw = (gu - h) + n
    f = T(np.float32(1.0001))
    e5, t40, t14 = T(np.float32(1e-5)), T(np.float32(2.0 ** -40)), T(np.float32(2.0 ** -14))

    def nrm(v):
        return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]) * f

    pn, pao = nrm(n), nrm(ao)
    pu, pv = nrm(e2) * pao, nrm(e1) * pao
    tiny = pn * t40
    C = {"n": n, "gu": gu, "h": h, "kw": kw,
         "m0": e5 * pn, "m1": e5 * pu + tiny, "m2": e5 * pv + tiny, "m3": e5 * ((pu + pv) + pn) + pn * t14,
         "g0": pn, "g1": np.maximum(nrm(gu), pu), "g2": np.maximum(nrm(h), pv), "g3": nrm(kw) + e5 * ((pu + pv) + pn)}
    return idx, mesh_of, C


def _near(v, thr):
    return np.abs(v - thr) <= BORDER * np.abs(thr)


def _span(ar, corners, C, sel):
    """min c.n, max c.gu, min c.h, min c.kw over corners [..., Q, 3] for the records sel -> [..., K] each."""
    c = corners[..., :, None, :]  # [..., Q, 1, 3]
    vn = ar.dot(c, C["n"][sel]).min(-2)
    vu = ar.dot(c, C["gu"][sel]).max(-2)
    vh = ar.dot(c, C["h"][sel]).min(-2)
    vw = ar.dot(c, C["kw"][sel]).min(-2)
    return vn, vu, vh, vw


def _reject(C, sel, vn, vu, vh, vw):
    rej = (vn > C["m0"][sel]) | (vu < -C["m1"][sel]) | (vh > C["m2"][sel]) | (vw > C["m3"][sel])
    near = _near(vn, C["m0"][sel]) | _near(vu, -C["m1"][sel]) | _near(vh, C["m2"][sel]) | _near(vw, C["m3"][sel])
    return rej, near


def tile_lists(pc, rays, tris, meshes, rule="pixel", mirror=False, sub=1):
    """The lists of every 8x8 tile of a pc.width x pc.height frame (no row partition).

    rule: "cap" (the parent's rule), "tile" (cap, then the tile box's corners), "pixel" (the product: cap,
    tile corners, then per pixel; sub > 1: sub x sub pixel boxes instead of single pixels).
    -> dict(n, ok, lists (global triangle indices, list order), border (per tile: the set of triangle
    indices some comparison of which was within BORDER of its threshold), tiles_x)."""
    ar = Arith(mirror)
    T = ar.T
    W, H = int(pc.width), int(pc.height)
    M = ar.a(np.array(pc.cam_alignment_mat[:], np.float32))
    j = T(np.float32(abs(np.float32(pc.jitter_size)))) * T(np.float32(1.0001))
    idx, _, C = camera_records(ar, np.array(pc.cam_pos[:], np.float32), tris, meshes[:int(pc.num_meshes)])
    cen = ar.a(rays["sample_centre"][:W * H, :3]).reshape(H, W, 3)
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    out = {"n": [], "ok": [], "lists": [], "border": [], "tiles_x": tiles_x}
    half, one5, one52 = T(0.5), T(np.float32(1.00001)), T(np.float32(1.00002))
    e5, e6 = T(np.float32(1e-5)), T(np.float32(1e-6))
    allsel = np.arange(idx.size)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            px = cen[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].reshape(-1, 3)
            lo, hi = px.min(0), px.max(0)
            axis = ar.box_dir(M, half * lo + half * hi)
            cor = np.array([[hi[0] if q & 1 else lo[0], hi[1] + j if q & 2 else lo[1] - j,
                             hi[2] + j if q & 4 else lo[2] - j] for q in range(8)], T)
            cdir = ar.box_dir(M, cor)
            c_lo = ar.dot(cdir, axis).min() - e5
            if not (c_lo > half) or int(pc.num_meshes) > 32:
                out["n"].append(0), out["ok"].append(False), out["lists"].append(np.zeros(0, np.int64))
                out["border"].append(set())
                continue
            s_hi = np.sqrt(max(T(0), one52 - c_lo * c_lo)) * one5 + e6

            def lower(ga, gn):
                return np.minimum(c_lo * ga, one5 * ga) - s_hi * gn

            def upper(ga, gn):
                return np.maximum(c_lo * ga, one5 * ga) + s_hi * gn

            vals = (lower(ar.dot(C["n"], axis), C["g0"]), upper(ar.dot(C["gu"], axis), C["g1"]),
                    lower(ar.dot(C["h"], axis), C["g2"]), lower(ar.dot(C["kw"], axis), C["g3"]))
            rej, near = _reject(C, allsel, *vals)
            border = set(idx[near].tolist())
            sel = allsel[~rej]
            if rule != "cap" and sel.size:
                q = cdir[::2] if lo[0] == hi[0] else cdir
                rej, near = _reject(C, sel, *_span(ar, q, C, sel))
                border |= set(idx[sel[near]].tolist())
                sel = sel[~rej]
            ok = sel.size <= CAP
            if ok and rule == "pixel" and sel.size:
                if sub > 1:  # sub x sub pixel boxes (the table's intermediate rows)
                    g = cen[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
                    boxes = [g[y:y + sub, x:x + sub].reshape(-1, 3) for y in range(0, g.shape[0], sub)
                             for x in range(0, g.shape[1], sub)]
                    blo = np.array([b.min(0) for b in boxes])
                    bhi = np.array([b.max(0) for b in boxes])
                else:
                    blo = bhi = px
                pcor = np.stack([np.stack([(bhi if q & 4 else blo)[:, 0], bhi[:, 1] + j if q & 1 else blo[:, 1] - j,
                                           bhi[:, 2] + j if q & 2 else blo[:, 2] - j], -1) for q in range(8 if sub > 1 else 4)], 1)
                rej, near = _reject(C, sel, *_span(ar, ar.box_dir(M, pcor), C, sel))  # [P, K]
                border |= set(idx[sel[near.any(0)]].tolist())
                sel = sel[~rej.all(0)]
            out["n"].append(int(sel.size) if ok else 0), out["ok"].append(bool(ok))
            out["lists"].append(idx[sel] if ok else np.zeros(0, np.int64)), out["border"].append(border)
    return out


# ---- float64 ground truth: which triangles a pixel's primary rays hit ---------------------------------

def ray_dirs(pc, centre, dy, dz):
    """get_ray_dir's float32 arithmetic for nc = (centre + (0, 0, dz)) + (0, dy, 0): [..., 3] float32."""
    ar = Arith(True)
    M = np.array(pc.cam_alignment_mat[:], np.float32)
    c = np.asarray(centre, np.float32)
    nc = np.stack([c[..., 0] + np.float32(0), (c[..., 1] + np.float32(0)) + np.float32(dy),
                   (c[..., 2] + np.float32(dz)) + np.float32(0)], -1).astype(np.float32)
    w = np.stack([ar.fma(M[8], nc[..., 2], ar.fma(M[4], nc[..., 1], M[0] * nc[..., 0])),
                  ar.fma(M[9], nc[..., 2], ar.fma(M[5], nc[..., 1], M[1] * nc[..., 0])),
                  ar.fma(M[10], nc[..., 2], ar.fma(M[6], nc[..., 1], M[2] * nc[..., 0]))], -1)
    return ar.normalize(w)


def hits(pc, tris, meshes, dirs, eps=1e-4, tmin=0.001):
    """Float64 Moller-Trumbore of the rays cam_pos + t dirs[r] (dirs: [R, 3]) against every camera-facing
    triangle of the first pc.num_meshes meshes -> the sorted global indices of the triangles that some ray
    hits with u, v, w >= eps and t > tmin.  Triangles whose direction cone (around their vertices'
    directions, float64, 1e-6 rad of slack) misses the rays' cone are skipped: they cannot be hit."""
    o = np.array(pc.cam_pos[:3], np.float64)
    k = np.concatenate([np.arange(int(r["first_index"]), int(r["first_index"]) + int(r["len"]))
                        for r in meshes[:int(pc.num_meshes)]] or [np.zeros(0, np.int64)])
    a, e1 = tris["a"][k, :3].astype(np.float64), tris["edge_one"][k, :3].astype(np.float64)
    e2, n = tris["edge_two"][k, :3].astype(np.float64), tris["normal"][k, :3].astype(np.float64)
    s = o - a
    facing = np.einsum("ij,ij->i", s, n) > 0
    k, a, e1, e2, n, s = k[facing], a[facing], e1[facing], e2[facing], n[facing], s[facing]
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    # cone prefilter
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)  # noqa: E731
    vd = np.stack([unit(a - o), unit(a + e1 - o), unit(a + e2 - o)], 1)  # [K, 3, 3]
    tax = vd.sum(1)
    tlen = np.linalg.norm(tax, axis=-1)
    tax = tax / np.maximum(tlen, 1e-300)[:, None]
    tcos = np.einsum("kvi,ki->kv", vd, tax).min(1)
    wide = (tlen < 1e-9) | (tcos <= 0.0)  # no usable cone: always a candidate
    rax = unit(d.sum(0))
    rcos = (d @ rax).min()
    ang = np.arccos(np.clip(tax @ rax, -1, 1))
    cand = wide | (rcos <= 0.0) | (ang <= np.arccos(np.clip(tcos, -1, 1)) + np.arccos(np.clip(rcos, -1, 1)) + 1e-6)
    k, a, e1, e2, n, s = k[cand], a[cand], e1[cand], e2[cand], n[cand], s[cand]
    if k.size == 0:
        return np.zeros(0, np.int64)
    D = d[:, None, :]
    hv = np.cross(D, e2[None])
    det = np.einsum("rki,ki->rk", hv, e1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 1.0 / det
        u = f * np.einsum("rki,ki->rk", hv, s)
        qv = np.cross(s, e1)
        v = f * np.einsum("rki,ki->rk", np.broadcast_to(D, hv.shape), qv)
        t = f * np.einsum("ki,ki->k", e2, qv)[None]
        front = np.einsum("rki,ki->rk", np.broadcast_to(D, hv.shape), n) < 0
        hit = front & (det > 0) & (u >= eps) & (v >= eps) & (1.0 - u - v >= eps) & (t > tmin)
    return np.sort(k[hit.any(0)])


def pixel_sample_offsets(jitter, seed):
    """(dy, dz) of a pixel's jitter-box corners, its centre and 8 seeded points inside the box."""
    jv = float(abs(np.float32(jitter)))
    pts = [(-jv, -jv), (jv, -jv), (-jv, jv), (jv, jv), (0.0, 0.0)]
    rng = np.random.default_rng(seed)
    pts += [tuple(p) for p in rng.uniform(-jv, jv, size=(8, 2))]
    return np.array(pts, np.float32)


def tile_hits(pc, rays, tris, meshes, seed=7):
    """Per 8x8 tile: the triangles hit by some sample ray (pixel_sample_offsets) of some pixel of the tile."""
    W, H = int(pc.width), int(pc.height)
    cen = rays["sample_centre"][:W * H, :3].reshape(H, W, 3)
    off = pixel_sample_offsets(pc.jitter_size, seed)
    out = []
    for ty in range((H + 7) // 8):
        for tx in range((W + 7) // 8):
            px = cen[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].reshape(-1, 1, 3)
            d = ray_dirs(pc, np.broadcast_to(px, (px.shape[0], off.shape[0], 3)), off[None, :, 0], off[None, :, 1])
            out.append(hits(pc, tris, meshes, d.reshape(-1, 3)))
    return out


def main(argv):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import SceneCase
    name = argv[1] if len(argv) > 1 else "island"
    size = (int(argv[2]), int(argv[3])) if len(argv) > 3 else (192, 108)
    mirror = "--mirror" in argv
    case = SceneCase(name, size)
    pc = case.push()
    truth = tile_hits(pc, case.rays, case.tris, case.meshes)
    print(f"{name} {size[0]}x{size[1]}, {'float32 mirror' if mirror else 'float64'}: "
          f"{sum(1 for t in truth if t.size)} tiles with a hit")
    print(f"{'rule':<28}{'non-sky tiles':>15}{'list entries':>15}{'hit tiles missed':>18}")
    for label, rule, sub in (("cap (parent)", "cap", 1), ("tile corners", "tile", 1), ("4x4 sub-boxes", "pixel", 4),
                             ("2x2 sub-boxes", "pixel", 2), ("per pixel (product)", "pixel", 1)):
        r = tile_lists(pc, case.rays, case.tris, case.meshes, rule=rule, mirror=mirror, sub=sub)
        nonsky = sum(1 for n, ok in zip(r["n"], r["ok"]) if n or not ok)
        missed = sum(1 for t, lst, ok in zip(truth, r["lists"], r["ok"]) if ok and np.setdiff1d(t, lst).size)
        print(f"{label:<28}{nonsky:>15}{sum(r['n']):>15}{missed:>18}")


if __name__ == "__main__":
    main(sys.argv)
