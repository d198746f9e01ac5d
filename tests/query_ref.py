"""Reference for the ray queries (hrt_intersect / hrt_intersect_primary): a Python world_hit
built from the oracle's exported intersecting_aabb / intersecting_tri, with the pieces the oracle does not
export -- the sphere test, the S4 normalise, the primary direction product, the sphere hit normal --
restated in binary32 with an exact fused multiply-add (the exact rational result rounded once; math.fma on
doubles would round twice).  Also the seeded ray families of tests/test_gpu_intersect.py.  Not a test.
"""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction

import numpy as np

import pyoracle
from helpers import _lib

F32 = np.float32
FLT_MAX = F32(3.402823466e+38)
T_MIN = F32(0.001)
NONE = 0xFFFFFFFF
BAND_TAU = 3e-3  # hrt_bvh.h kBandTau: the grazing band's width in d.n^


# ---- binary32 arithmetic -------------------------------------------------------------------------------

def round_f32(q: Fraction, negative_zero: bool = False) -> np.float32:
    """q rounded to the nearest binary32, ties to even, denormals kept, overflow to infinity."""
    if q == 0:
        return F32(-0.0) if negative_zero else F32(0.0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if a < Fraction(2) ** e:
        e -= 1
    elif a >= Fraction(2) ** (e + 1):
        e += 1
    ue = max(e, -126) - 23
    n = round(a / Fraction(2) ** ue)  # Fraction.__round__: half to even
    if n * Fraction(2) ** ue >= Fraction(2) ** 128:
        v = math.inf
    else:
        v = math.ldexp(n, ue)
    return F32(-v if q < 0 else v)


def fma32(a, b, c) -> np.float32:
    """RN(a * b + c) of three binary32 values, rounded once."""
    a, b, c = float(F32(a)), float(F32(b)), float(F32(c))
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))  # inf / NaN rules only
    p = Fraction(a) * Fraction(b)
    s = p + Fraction(c)
    if s == 0:
        pneg = math.copysign(1.0, a) * math.copysign(1.0, b) < 0
        # an exact zero sum is +0 unless both addends are negative zeros
        return round_f32(s, p == 0 and c == 0 and pneg and math.copysign(1.0, c) < 0)
    return round_f32(s)


def mul32(a, b) -> np.float32:
    with np.errstate(all="ignore"):
        return F32(F32(a) * F32(b))


def dot32(a, b) -> np.float32:
    """S2: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    return fma32(a[2], b[2], fma32(a[1], b[1], mul32(a[0], b[0])))


def cross32(a, b):
    with np.errstate(all="ignore"):
        return [fma32(a[1], b[2], -mul32(a[2], b[1])), fma32(a[2], b[0], -mul32(a[0], b[2])),
                fma32(a[0], b[1], -mul32(a[1], b[0]))]


def normalize32(v):
    """S4: v / sqrt(dot(v, v)), correctly rounded root and quotients.  Returns (unit vector, dot(v, v))."""
    d2 = dot32(v, v)
    with np.errstate(all="ignore"):
        l = np.sqrt(d2, dtype=F32)
        return np.array([F32(v[0]) / l, F32(v[1]) / l, F32(v[2]) / l], F32), d2


def regular(o, d_unit, d2) -> bool:
    """S11: a ray the hierarchy methods traverse (finite origin, a finite unit direction); the others are
    answered by the literal scan and counted in hrt_query_stats.scan_rays."""
    return bool(np.all(np.isfinite(o)) and np.all(np.isfinite(d_unit)) and d2 >= F32(2.0) ** -126 and d2 <= FLT_MAX)


def tri_dist32(tri, o, d) -> np.float32:
    """intersecting_tri's distance (raytracing.glsl:213-241) restated with the exact fma: FLT_MAX for a miss."""
    n, a = tri["normal"][:3], tri["a"][:3]
    dn = dot32(d, n)
    if dn >= 0:
        return FLT_MAX
    with np.errstate(all="ignore"):
        ao = [F32(o[k]) - F32(a[k]) for k in range(3)]
        dao = cross32(ao, d)
        det = -dn
        if det == 0:
            return FLT_MAX
        inv = F32(1.0) / det
        dist = dot32(ao, n) * inv
        if dist < 0:
            return FLT_MAX
        u = dot32(tri["edge_two"][:3], dao) * inv
        if u < 0:
            return FLT_MAX
        v = -dot32(tri["edge_one"][:3], dao) * inv
        if v < 0:
            return FLT_MAX
        if F32(1.0) - u - v < 0:
            return FLT_MAX
        return F32(dist)


def sphere_dist32(s, o, d) -> np.float32:
    """intersecting_sphere's distance (raytracing.glsl:169-190), the near root; FLT_MAX for a miss."""
    with np.errstate(all="ignore"):
        l = [F32(o[k]) - F32(s["centre"][k]) for k in range(3)]
        a = dot32(d, d)
        half_b = dot32(d, l)
        c = dot32(l, l) - mul32(s["radius"], s["radius"])
        disc = mul32(half_b, half_b) - mul32(a, c)
        if disc >= 0:
            return F32((-half_b - np.sqrt(disc, dtype=F32)) / a)
    return FLT_MAX


# ---- world_hit ---------------------------------------------------------------------------------------

class QueryScene:
    """The records of a helpers.SceneCase laid out for the oracle's exported functions."""

    def __init__(self, case):
        self.case = case
        self.tris = np.ascontiguousarray(case.tris)
        self.meshes = np.ascontiguousarray(case.meshes)
        self.spheres = np.ascontiguousarray(case.spheres)
        self.lib = pyoracle.load()
        self.tri_base = self.tris.ctypes.data
        self.mn = [np.ascontiguousarray(m["min_point"], F32) for m in self.meshes]
        self.mx = [np.ascontiguousarray(m["max_point"], F32) for m in self.meshes]
        self.oracle_calls = 0
        pts = [m for m in self.mn] + [m for m in self.mx]
        for s in self.spheres:
            pts += [s["centre"] - s["radius"], s["centre"] + s["radius"]]
        pts = np.array(pts, np.float64) if pts else np.zeros((2, 3))
        self.lo, self.hi = pts.min(0), pts.max(0)
        self.centre = (0.5 * (self.lo + self.hi)).astype(F32)
        self.diagonal = float(np.linalg.norm(self.hi - self.lo))

    def world_hit(self, o, d_raw, t_max=FLT_MAX, n_spheres=None, n_meshes=None):
        """S11 for one ray -> (t, kind, index, mesh, normal[3], tri_tests, answered by the scan fallback)."""
        ns = len(self.spheres) if n_spheres is None else n_spheres
        nm = len(self.meshes) if n_meshes is None else n_meshes
        o = np.ascontiguousarray(o, F32)
        d, d2 = normalize32(np.asarray(d_raw, F32))
        d = np.ascontiguousarray(d)
        miss = (FLT_MAX, 0, NONE, NONE, np.zeros(3, F32), 0, False)
        t_max = F32(t_max)
        if not t_max > T_MIN:  # NaN or <= 0.001: a certain miss, nothing tested
            return miss
        closest = (min(t_max, FLT_MAX), 0, NONE, NONE, np.zeros(3, F32))
        for i in range(ns):  # raytracing.glsl:271-276
            t = sphere_dist32(self.spheres[i], o, d)
            if t > T_MIN and t < closest[0]:
                with np.errstate(all="ignore"):
                    pos = o + d * t
                    nrm, _ = normalize32(pos - self.spheres[i]["centre"])
                closest = (t, 1, i, NONE, nrm)
        tests = 0
        out = np.zeros(4, F32)
        P = ctypes.c_void_p
        op, dp, outp = P(o.ctypes.data), P(d.ctypes.data), P(out.ctypes.data)
        for m in range(nm):  # raytracing.glsl:277-286, intersecting_mesh :243-264
            if not self.lib.orc_intersecting_aabb(P(self.mn[m].ctypes.data), P(self.mx[m].ctypes.data), op, dp):
                continue
            first, ln = int(self.meshes[m]["first_index"]), int(self.meshes[m]["len"])
            tests += ln
            best = (FLT_MAX, NONE, None)
            for i in range(first, first + ln):
                self.lib.orc_intersecting_tri(P(self.tri_base + 64 * i), op, dp, outp)
                if out[3] > T_MIN and out[3] < best[0]:
                    best = (F32(out[3]), i, out[:3].copy())
            self.oracle_calls += ln
            if best[0] > T_MIN and best[0] < closest[0]:
                closest = (best[0], 2, best[1], m, best[2])
        if closest[1] == 0:
            return miss[:5] + (tests, not regular(o, d, d2))
        return closest + (tests, not regular(o, d, d2))

    def hits(self, rays, n_spheres=None, n_meshes=None):
        """-> (hits as _lib.HIT_DTYPE, sum of tri_tests, rays the scan fallback answers)."""
        out = np.zeros(len(rays), dtype=_lib.HIT_DTYPE)
        tests = scans = 0
        for k, r in enumerate(rays):
            t, kind, idx, mesh, nrm, tt, scan = self.world_hit(r["origin"], r["direction"], r["t_max"], n_spheres, n_meshes)
            out[k] = (t, kind, idx, mesh, nrm, 0)
            tests += tt
            scans += int(scan)
        return out, tests, scans


def count_irregular(rays) -> int:
    """The rays of a batch that S11 sends to the literal scan (and counts in scan_rays).  Rays whose squared
    length is far inside the normal range in double precision and whose components are all finite are regular;
    only the others take the exact binary32 rule."""
    o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)
    with np.errstate(all="ignore"):
        d2 = (d * d).sum(1)
        clear = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d2 > 1e-30) & (d2 < 1e30)
    n = 0
    for r in rays[~clear]:
        if not F32(r["t_max"]) > T_MIN:
            continue
        d, d2 = normalize32(r["direction"])
        n += 0 if regular(r["origin"], d, d2) else 1
    return n


# ---- rays ----------------------------------------------------------------------------------------------

def make_rays(origins, directions, t_max=None):
    o = np.asarray(origins, F32).reshape(-1, 3)
    d = np.asarray(directions, F32).reshape(-1, 3)
    rays = np.zeros(len(o), dtype=_lib.RAY_QUERY_DTYPE)
    rays["origin"], rays["direction"] = o, d
    rays["t_max"] = FLT_MAX if t_max is None else np.asarray(t_max, F32)
    return rays


def primary_rays(case, pc, xs, ys):
    """The rays hrt_intersect_primary builds for pixels (xs, ys): origin cam_pos, direction mat3(M) c with
    get_ray_dir's row-wise product (left for hrt_intersect to normalise), t_max FLT_MAX."""
    M = [F32(v) for v in pc.cam_alignment_mat]
    W = int(pc.width)
    dirs = []
    for x, y in zip(xs, ys):
        c = case.rays["sample_centre"][int(x) + int(y) * W]
        dirs.append([fma32(M[8 + k], c[2], fma32(M[4 + k], c[1], mul32(M[k], c[0]))) for k in range(3)])
    o = np.tile(np.array([pc.cam_pos[0], pc.cam_pos[1], pc.cam_pos[2]], F32), (len(dirs), 1))
    return make_rays(o, np.array(dirs, F32).reshape(-1, 3))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _tri_points(qs, rng, n, lo=0.0, hi=1.0):
    """n (triangle index, point a + u e1 + v e2) with u, v drawn from [lo, hi] (inside when lo = 0, hi = 1)."""
    T = qs.tris
    if len(qs.meshes) == 0:  # a scene of spheres only: points on their surfaces (index 0: the null triangle)
        k = rng.integers(0, len(qs.spheres), n)
        p = qs.spheres["centre"][k].astype(np.float64) + qs.spheres["radius"][k, None] * _unit(rng, n)
        return np.zeros(n, np.int64), p
    idx = rng.integers(0, len(T), n)
    u, v = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    if lo == 0.0 and hi == 1.0:
        fold = u + v > 1
        u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
    p = T["a"][idx, :3].astype(np.float64) + u[:, None] * T["edge_one"][idx, :3] + v[:, None] * T["edge_two"][idx, :3]
    return idx, p


def family(qs: QueryScene, name: str, n: int, seed: int, pc=None):
    """n seeded rays of family `name` (a-f, h, i) for the scene; (g) needs a first pass: t_max_family."""
    rng = np.random.default_rng([seed, ord(name)])
    T = qs.tris
    span = np.maximum(qs.hi - qs.lo, 1e-3)
    if name == "a":  # pixel-centre rays of the camera
        W, H = int(pc.width), int(pc.height)
        p = rng.integers(0, W * H, n)
        return primary_rays(qs.case, pc, p % W, p // W)
    if name == "b":  # origin on a random triangle, random direction
        _, p = _tri_points(qs, rng, n)
        return make_rays(p, _unit(rng, n))
    if name == "c":  # origin and direction both in a triangle's plane (some origins outside the triangle)
        idx, p = _tri_points(qs, rng, n, -1.0, 2.0)
        al, be = rng.normal(size=n), rng.normal(size=n)
        d = al[:, None] * T["edge_one"][idx, :3].astype(np.float64) + be[:, None] * T["edge_two"][idx, :3]
        d[::4] = T["edge_one"][idx[::4], :3]  # along an edge exactly
        p[1::8] = T["a"][idx[1::8], :3]       # from a vertex exactly
        # every third ray: just outside the grazing band instead -- tilted out of the plane by d.n^ = -k tau_g
        # (k from 0.9 to 3: either side of the band's edge, where the node margins ~ 1 / (tau_g - rho) are
        # thinnest against the error of u and v), aimed within 1e-7 .. 1e-3 triangle extents of an edge, on
        # either side of it, from half a scene diagonal to 1e3 diagonals away
        g = np.flatnonzero(np.arange(n) % 3 == 2)
        e1, e2 = T["edge_one"][idx[g], :3].astype(np.float64), T["edge_two"][idx[g], :3].astype(np.float64)
        nrm = np.cross(e1, e2)
        ln = np.linalg.norm(nrm, axis=1)
        ok = ln > 1e-20
        g, e1, e2, nrm = g[ok], e1[ok], e2[ok], nrm[ok] / ln[ok, None]
        m = len(g)
        a = T["a"][idx[g], :3].astype(np.float64)
        s = rng.uniform(0, 1, m)[:, None]
        edge = rng.integers(0, 3, m)[:, None]
        on_edge = np.where(edge == 0, a + s * e1, np.where(edge == 1, a + s * e2, a + e1 + s * (e2 - e1)))
        along = np.where(edge == 0, e1, np.where(edge == 1, e2, e2 - e1))
        out = np.cross(along, nrm) * np.where(edge == 1, -1.0, 1.0)  # in the plane, pointing out of the triangle
        out /= np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-300)
        ext = np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1))[:, None]
        sin_t = BAND_TAU * rng.choice([0.9, 0.99, 1.01, 1.1, 1.5, 3.0], m)[:, None]
        far = rng.choice([0.5, 10.0, 1e3], m)[:, None] * qs.diagonal
        off = rng.choice([-1.0, 1.0], m)[:, None] * 10.0 ** rng.uniform(-7, -3, m)[:, None] * ext
        # ... and every other one of them by the size of the reference's own error instead: the rounding of
        # o - a (an ulp of |o|) seen through 1 / |d.n^| moves the computed (u, v) by about noise below, so the
        # reference accepts some rays that pass that far OUTSIDE the triangle -- outside its leaf's plain box:
        # the hits the margins' b R term exists for
        noise = 6e-8 * (far + np.linalg.norm(on_edge, axis=1, keepdims=True)) / sin_t
        wide = (np.arange(m) % 2 == 1)[:, None]
        off = np.where(wide, rng.choice([-1.0, 1.0], m)[:, None] * 10.0 ** rng.uniform(-2, 0.3, m)[:, None] * noise, off)
        tgt = on_edge + out * off
        u = al[g, None] * e1 + be[g, None] * e2
        u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-300)
        dg = u * np.sqrt(1.0 - sin_t ** 2) - nrm * sin_t
        p[g], d[g] = tgt - dg * far, dg
        return make_rays(p, d)
    if name == "i":  # the node margins' b R term: near-band rays from 1e4 / 1e5 scene diagonals, just off an edge
        # At that distance o - a rounds to an ulp of |o|, which 1 / |d.n^| turns into an in-plane shift of about
        # `noise`; the reference then accepts rays that pass up to that far outside a triangle, outside its
        # leaf's box grown by the margins' a term alone.  Aimed 0.01 .. 0.3 noise off an edge (either side),
        # d.n^ = -k tau_g with k in {1.02, 1.1, 1.5}: with the b R term dropped about 1 ray in 5,000 of these
        # gets a wrong answer from either traversal on island and cave (profiles/query_mutants.txt).
        idx = rng.integers(0, len(T), n)
        e1, e2 = T["edge_one"][idx, :3].astype(np.float64), T["edge_two"][idx, :3].astype(np.float64)
        nrm = np.cross(e1, e2)
        ln = np.linalg.norm(nrm, axis=1, keepdims=True)
        flat = ln[:, 0] <= 1e-12  # (zero-area triangles: any in-plane pair will do)
        nrm = np.where(flat[:, None], [0.0, 1.0, 0.0], nrm / np.maximum(ln, 1e-300))
        a = T["a"][idx, :3].astype(np.float64)
        s = rng.uniform(0, 1, n)[:, None]
        edge = rng.integers(0, 3, n)[:, None]
        on_edge = np.where(edge == 0, a + s * e1, np.where(edge == 1, a + s * e2, a + e1 + s * (e2 - e1)))
        along = np.where(edge == 0, e1, np.where(edge == 1, e2, e2 - e1))
        out = np.cross(along, nrm) * np.where(edge == 1, -1.0, 1.0)
        out /= np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-300)
        sin_t = BAND_TAU * rng.choice([1.02, 1.1, 1.5], n)[:, None]
        far = rng.choice([1e4, 1e5], n)[:, None] * qs.diagonal
        noise = 6e-8 * (far + np.linalg.norm(on_edge, axis=1, keepdims=True)) / sin_t
        tgt = on_edge + out * rng.choice([-1.0, 1.0], n)[:, None] * 10.0 ** rng.uniform(-2, -0.5, n)[:, None] * noise
        u = rng.normal(size=n)[:, None] * e1 + rng.normal(size=n)[:, None] * e2
        u = np.where(flat[:, None], [1.0, 0.0, 0.0], u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-300))
        dg = u * np.sqrt(1.0 - sin_t ** 2) - nrm * sin_t
        return make_rays(tgt - dg * far, dg)
    if name == "d":  # aimed exactly at a vertex / at an edge midpoint (shared by the neighbouring triangles)
        idx = rng.integers(0, len(T), n)
        a, e1, e2 = T["a"][idx, :3], T["edge_one"][idx, :3], T["edge_two"][idx, :3]
        pick = rng.integers(0, 6, n)[:, None]
        half = F32(0.5)
        tgt = np.where(pick == 0, a, np.where(pick == 1, a + e1, np.where(pick == 2, a + e2, np.where(
            pick == 3, a + half * e1, np.where(pick == 4, a + half * e2, (a + e1) + half * (e2 - e1)))))).astype(F32)
        o = (qs.centre + (rng.uniform(-0.75, 0.75, (n, 3)) * span)).astype(F32)
        return make_rays(o, tgt - o)  # the binary32 difference: the target lies on the ray up to that rounding
    if name == "e":  # the six axis directions, and directions with one or two zero components
        d = _unit(rng, n)
        k = np.arange(n)
        axis = np.zeros((n, 3))
        axis[k, k % 3] = np.where((k // 3) % 2 == 0, 1.0, -1.0)
        third = k % 3 == 0
        d[third] = axis[third]
        one_zero = k % 3 == 1
        d[one_zero, rng.integers(0, 3, n)[one_zero]] = 0.0
        two_zero = k % 6 == 2
        d[two_zero] = axis[two_zero] * rng.uniform(0.1, 3.0, n)[two_zero, None]
        neg = k % 4 == 3
        d[neg] = np.where(d[neg] == 0.0, -0.0, d[neg])  # negative zeros select the other AABB corner
        _, p = _tri_points(qs, rng, n)
        o = np.where((k % 2 == 0)[:, None], p, qs.centre + rng.uniform(-0.6, 0.6, (n, 3)) * span)
        return make_rays(o, d)
    if name == "f":  # origins 1e3 and 1e6 scene diagonals away aimed at the scene; origins at the box centre
        k = np.arange(n)
        tgt = qs.centre + rng.uniform(-0.5, 0.5, (n, 3)) * span
        u = _unit(rng, n)
        dist = np.where(k % 3 == 0, 1e3, 1e6) * qs.diagonal
        o = tgt - u * dist[:, None]
        d = tgt - o.astype(F32)
        mid = k % 3 == 2
        o[mid] = qs.centre
        d[mid] = _unit(rng, n)[mid]
        return make_rays(o, d)
    if name == "h":  # non-finite origins, zero / underflowing directions, NaN / negative / tiny t_max
        base = family(qs, "b", n, seed + 1)
        k = np.arange(n)
        o, d, t = base["origin"].copy(), base["direction"].copy(), base["t_max"].copy()
        o[k % 8 == 0, 0] = np.nan
        o[k % 8 == 1, 1] = np.inf
        o[k % 8 == 2, 2] = -np.inf
        d[k % 8 == 3] = 0.0
        d[k % 8 == 4] *= F32(1e-30)
        t[k % 8 == 5] = np.nan
        t[k % 8 == 6] = -1.0
        t[k % 8 == 7] = np.where(k[k % 8 == 7] % 16 == 7, F32(0.001), F32(0.0005))
        t[k % 32 == 0] = np.nan  # a certain miss comes first: not a scan ray either
        d[k % 64 == 35] = F32(3e19)  # dot(d, d) overflows: d / inf is a finite zero vector, not a direction
        return make_rays(o, d, t)
    raise ValueError(name)


def t_max_family(rays, hits, n: int, seed: int):
    """(g): rays of a first pass that hit, with t_max set to the exact t returned, its next float up and its
    next float down (thirds of the batch)."""
    rng = np.random.default_rng([seed, ord("g")])
    hit = np.flatnonzero(hits["kind"] != 0)
    if len(hit) == 0:
        return rays[:0].copy()
    sel = hit[rng.integers(0, len(hit), n)]
    out = rays[sel].copy()
    t = hits["t"][sel].astype(F32)
    k = np.arange(n)
    out["t_max"] = np.where(k % 3 == 0, t, np.where(k % 3 == 1, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(0))))
    return out
