"""Radiance queries (hrt_radiance): the reference and the query families.  A helper, not
a test.

The reference is the oracle's orc_trace_pixel on a 1 x 1 image: width = height = num_rays = 1, rays[0] = the
query's centre, cam_pos = its origin, rng_offset = seed * 719393^-1 mod 2^32 -- so that main()'s state
rng_offset * 719393 + 0 is the seed.  It returns the pre-quantisation rgb and that query's segments and triangle
tests (tests/test_radiance_ref.py pins the construction to whole oracle frames)."""
import numpy as np

import pyoracle
import query_ref as Q
from helpers import _lib

F32 = np.float32
SEED_MUL = 719393
SEED_INV = pow(SEED_MUL, -1, 1 << 32)  # 719393 is odd: the seed map is a bijection on uint32
assert SEED_MUL * SEED_INV % (1 << 32) == 1


def copy_push(pc, **fields):
    out = _lib.PushConstants.from_buffer_copy(pc)
    for k, v in fields.items():
        setattr(out, k, v)
    return out


def make_queries(origins, seeds, centres):
    o = np.asarray(origins, F32).reshape(-1, 3)
    q = np.zeros(len(o), dtype=_lib.RADIANCE_QUERY_DTYPE)
    q["origin"], q["centre"] = o, np.asarray(centres, F32).reshape(-1, 3)
    q["seed"] = np.asarray(seeds, np.uint32)
    return q


def oracle(case, pc, queries):
    """-> (rgba float32 (n, 4) as main() stores it, segments[n], tri_tests[n]) of the queries under pc."""
    n = len(queries)
    rgba = np.ones((n, 4), F32)
    seg, tests = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    one = copy_push(pc, width=1, height=1, num_rays=1)
    ray = np.zeros(1, dtype=_lib.RAY_DTYPE)
    for k, q in enumerate(queries):
        one.cam_pos[0], one.cam_pos[1], one.cam_pos[2] = (float(v) for v in q["origin"])
        one.rng_offset = int(q["seed"]) * SEED_INV % (1 << 32)
        ray["sample_centre"][0, :3] = q["centre"]
        rgba[k, :3], seg[k], tests[k] = pyoracle.trace_pixel(one, ray, case.spheres, case.tris, case.meshes, 0, 0)
    return rgba, seg, tests


def pixel_queries(case, pc, xs, ys):
    """The queries of pixels (xs, ys) of the frame pc traces."""
    ids = np.asarray(xs, np.int64) + np.asarray(ys, np.int64) * int(pc.width)
    seeds = (int(pc.rng_offset) * SEED_MUL + ids) % (1 << 32)
    o = np.tile(np.array([pc.cam_pos[0], pc.cam_pos[1], pc.cam_pos[2]], F32), (len(ids), 1))
    return make_queries(o, seeds, case.rays["sample_centre"][ids, :3])


def centres_for(pc, directions):
    """The centres whose un-jittered direction mat3(M) c is the given one (w_k = sum_j M[4 j + k] c_j)."""
    A = np.array([[pc.cam_alignment_mat[4 * j + k] for j in range(3)] for k in range(3)], np.float64)
    return np.linalg.solve(A, np.asarray(directions, np.float64).T).T.astype(F32)


def families(case, qs, pc, per_family, seed):
    """{family: queries}, seeded: `camera` pixels of the frame; `surface` origins on random triangles pushed off
    along the normal, random centres; `far` origins 1e3 and 1e6 scene diagonals away aimed at the scene; `seeds` 0
    and 0xFFFFFFFF on camera and surface records; `irregular` NaN and inf origins, NaN and inf centres (every
    segment of such a query fails S11's test), and a zero centre (regular unless the jitter is 0)."""
    rng = np.random.default_rng([seed, 13])
    W, H = int(pc.width), int(pc.height)
    out = {}
    p = rng.integers(0, W * H, per_family)
    out["camera"] = pixel_queries(case, pc, p % W, p // W)
    idx, pts = Q._tri_points(qs, rng, per_family)
    if len(qs.meshes):
        nrm = np.cross(qs.tris["edge_one"][idx, :3].astype(np.float64), qs.tris["edge_two"][idx, :3].astype(np.float64))
        ln = np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm = np.where(ln > 1e-20, nrm / np.maximum(ln, 1e-300), Q._unit(rng, per_family))
    else:
        nrm = pts - qs.spheres["centre"][0].astype(np.float64)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    side = np.where(rng.integers(0, 2, per_family)[:, None] == 0, 1.0, -1.0)
    out["surface"] = make_queries(pts + side * nrm * (1e-3 * qs.diagonal), rng.integers(0, 1 << 32, per_family),
                                  Q._unit(rng, per_family))
    n_far = per_family // 2
    u = Q._unit(rng, n_far)
    dist = np.where(np.arange(n_far) % 2 == 0, 1e3, 1e6)[:, None] * qs.diagonal
    target = qs.lo + rng.uniform(0, 1, (n_far, 3)) * (qs.hi - qs.lo)
    origin = target + u * dist
    aim = (target - origin) / np.linalg.norm(target - origin, axis=1, keepdims=True)
    out["far"] = make_queries(origin, rng.integers(0, 1 << 32, n_far), centres_for(pc, aim))
    n_seed = per_family // 4
    s = np.concatenate([out["camera"][:n_seed], out["surface"][:n_seed]]).copy()
    s["seed"] = np.where(np.arange(len(s)) % 2 == 0, 0, 0xFFFFFFFF)
    out["seeds"] = s
    k = 40
    irr = np.concatenate([out["camera"][:k], out["surface"][:k]]).copy()
    kind = np.arange(len(irr)) % 5
    irr["origin"][kind == 0, 0] = np.nan
    irr["origin"][kind == 1, 1] = np.inf
    irr["centre"][kind == 2, 2] = np.nan
    irr["centre"][kind == 3, 0] = -np.inf
    irr["centre"][kind == 4] = 0.0
    out["irregular"] = irr
    return out


def always_irregular(queries):
    """The queries every segment of which fails S11's test whatever pc's matrix and jitter: a non-finite origin
    stays non-finite along the path, and a non-finite centre gives a NaN direction in every sample."""
    return ~(np.isfinite(queries["origin"]).all(1) & np.isfinite(queries["centre"]).all(1))


def _differs(got, want):
    """Per element: the bits differ, except that a NaN equals a NaN (their payloads are the machine's)."""
    g, w = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert g.shape == w.shape, (g.shape, w.shape)
    return (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))


def same_bits(got, want):
    return not _differs(got, want).any()


def explain(got, want, queries):
    bad = np.flatnonzero(_differs(got, want).reshape(len(queries), -1).any(1))
    if bad.size == 0:
        return "identical"
    k = int(bad[0])
    return f"{bad.size} of {len(queries)} results differ; first at query {k} {queries[k]}: got {got[k]}, want {want[k]}"
