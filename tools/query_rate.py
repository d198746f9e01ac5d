#!/usr/bin/env python3
"""Ray-query rates (hrt_intersect / hrt_intersect_primary) on a scene, per method:

  primary   the whole image's un-jittered primary rays (hrt_intersect_primary), hits in device memory;
  bounce    N bounce-like rays (origin on a random triangle, random unit direction), rays and hits in
            device memory.

Per workload the methods take turns: two warm-up calls each, then `--repeat` timed rounds in which every
method runs once (so a drift of the machine hits all three alike).  A call is blocking (it ends in a stream
synchronise), so the host clock around it is the call's time: launch, kernel(s), synchronise.  The hits of
BVH and PAIRS are compared with SCAN's bytes before anything is reported.  One JSON line per (workload,
method): median / min / max milliseconds and Mrays/s from the median, plus the ratio to SCAN.

    python tools/query_rate.py --scene island --size 1920 1080 --rays 1000000 --out profiles/query_rate.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import epq_raytracer_amd as E  # noqa: E402
from epq_raytracer_amd import _lib  # noqa: E402

METHODS = (_lib.QUERY_SCAN, _lib.QUERY_BVH, _lib.QUERY_PAIRS)


class DevBuf:
    def __init__(self, hip, nbytes):
        p = ctypes.c_void_p()
        if hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) != 0:
            raise RuntimeError("hipMalloc failed (no device?)")
        self.hip, self.ptr, self.nbytes = hip, int(p.value), nbytes

    def write(self, a):
        a = np.ascontiguousarray(a)
        if self.hip.hipMemcpy(ctypes.c_void_p(self.ptr), ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes), 1) != 0:
            raise RuntimeError("hipMemcpy to the device failed")

    def read(self):
        out = np.empty(self.nbytes, np.uint8)
        if self.hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(self.ptr), ctypes.c_size_t(self.nbytes), 2) != 0:
            raise RuntimeError("hipMemcpy from the device failed")
        return out


def bounce_like_rays(tris, n, seed):
    """n rays with their origin on a random triangle (uniform over triangles, then over the triangle) and a
    uniformly random unit direction."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(tris), n)
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
    o = tris["a"][idx, :3] + u[:, None] * tris["edge_one"][idx, :3] + v[:, None] * tris["edge_two"][idx, :3]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return E.HrtContext.ray_queries(o, d)


def measure(calls, repeat, warmup=2):
    """calls: {method: callable}.  -> {method: [ms per timed call]}"""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    ms = {m: [] for m in calls}
    for _ in range(repeat):
        for m, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ms[m].append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="island")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()

    hip = ctypes.CDLL("libamdhip64.so")
    camera, settings = E.preset(args.scene)
    W, H = args.size
    ctx = E.HrtContext((W, H), device=args.device)
    pipe = E.RayTracePipeline(ctx, (W, H), settings)
    pc = pipe.push_constants(camera, 0, False)
    info = ctx.scene_info()
    lines = []

    def report(workload, n, ms, ran):
        scan = statistics.median(ms[_lib.QUERY_SCAN])
        for m in METHODS:
            med = statistics.median(ms[m])
            rec = {"tool": "query_rate", "build_id": _lib.build_id(), "scene": args.scene, "workload": workload,
                   "size": [W, H], "rays": n, "method": _lib.QUERY_NAMES[m], "method_ran": _lib.QUERY_NAMES[ran[m]],
                   "calls": len(ms[m]), "ms_median": round(med, 4), "ms_min": round(min(ms[m]), 4),
                   "ms_max": round(max(ms[m]), 4), "mrays_per_s": round(n / med / 1e3, 2),
                   "speedup_vs_scan": round(scan / med, 3), "bvh_built": info["bvh_built"], "triangles": len(pipe.tris)}
            lines.append(rec)
            print(json.dumps(rec))

    # primary: the whole image, hits in device memory
    n = W * H
    hits = {m: DevBuf(hip, n * 32) for m in METHODS}
    ran = {}

    def primary(m):
        st = _lib.QueryStats()
        ctx._check(ctx.lib.hrt_intersect_primary(ctx.handle, ctypes.byref(pc), 0, 0, W, H, m, ctypes.c_void_p(hits[m].ptr),
                                                 ctypes.byref(st)), "hrt_intersect_primary")
        ran[m] = st.method_ran

    ms = measure({m: (lambda m=m: primary(m)) for m in METHODS}, args.repeat)
    ref = hits[_lib.QUERY_SCAN].read()
    for m in METHODS[1:]:
        if not np.array_equal(hits[m].read(), ref):
            raise RuntimeError(f"primary: {_lib.QUERY_NAMES[m]} differs from scan")
    report("primary", n, ms, dict(ran))

    # bounce-like rays, rays and hits in device memory
    n = args.rays
    rays = bounce_like_rays(pipe.tris, n, args.seed)
    d_rays = DevBuf(hip, rays.nbytes)
    d_rays.write(rays)
    hits = {m: DevBuf(hip, n * 32) for m in METHODS}

    def bounce(m):
        ran[m] = ctx.intersect_into(d_rays.ptr, n, hits[m].ptr, m, with_stats=True).method_ran

    ms = measure({m: (lambda m=m: bounce(m)) for m in METHODS}, args.repeat)
    ref = hits[_lib.QUERY_SCAN].read()
    for m in METHODS[1:]:
        if not np.array_equal(hits[m].read(), ref):
            raise RuntimeError(f"bounce: {_lib.QUERY_NAMES[m]} differs from scan")
    report("bounce", n, ms, dict(ran))
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
