#!/usr/bin/env python3
"""Occlusion-query rates (hrt_occluded) against hrt_intersect on the same rays and the same
method, per scene:

  primary   the whole image's un-jittered primary rays, given as caller rays (t_max = FLT_MAX);
  bounce    N bounce-like rays (origin on a random triangle, random unit direction, t_max = FLT_MAX);
  segment   N surface-to-surface segments (both ends on random triangles; origin a, direction b - a,
            t_max = |b - a| as RayTracePipeline.segment_rays builds them).

Rays, hits and bits live in device memory.  Per workload the six calls (three methods x {occluded, intersect})
take turns: two warm-up calls each, then `--repeat` timed rounds in which every call runs once, so a drift of
the machine hits all alike.  A call is blocking (it ends in a stream synchronise), so the host clock around it
is the call's time.  Before anything is reported every method's bits are compared with kind != 0 of SCAN's
hits.  One JSON line per (workload, method): median / min / max milliseconds of both calls, Mrays/s from the
medians, and occluded's speed-up over intersect.

    python tools/occlusion_rate.py --scene island --size 1920 1080 --rays 1000000 --out profiles/occlusion_rate.jsonl

`--tag` labels the records (the no-early-exit experiment, tools/exp/occluded_no_early_exit.patch, is measured
with HRT_LIB pointing at its build and --tag no_early_exit)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import epq_raytracer_amd as E  # noqa: E402
from epq_raytracer_amd import _lib  # noqa: E402
from query_rate import METHODS, DevBuf, bounce_like_rays, measure  # noqa: E402


def surface_points(tris, n, rng):
    idx = rng.integers(0, len(tris), n)
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
    return tris["a"][idx, :3] + u[:, None] * tris["edge_one"][idx, :3] + v[:, None] * tris["edge_two"][idx, :3]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="island")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tag", default="product")
    ap.add_argument("--stats", action="store_true", help="time the calls with their statistics requested")
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

    # the primary rays as caller rays: origin cam_pos, direction mat3(M) c (float32; the library normalises)
    M = np.array(list(pc.cam_alignment_mat), np.float32).reshape(4, 4)
    c = ctx.read_rays().view(np.float32).reshape(-1, 4)[:W * H, :3]
    primary = E.HrtContext.ray_queries(np.tile(np.array(list(pc.cam_pos)[:3], np.float32), (W * H, 1)), c @ M[:3, :3])
    rng = np.random.default_rng([args.seed, 2])
    workloads = (("primary", primary), ("bounce", bounce_like_rays(pipe.tris, args.rays, args.seed)),
                 ("segment", E.RayTracePipeline.segment_rays(surface_points(pipe.tris, args.rays, rng),
                                                             surface_points(pipe.tris, args.rays, rng))))
    for workload, rays in workloads:
        n = len(rays)
        d_rays = DevBuf(hip, rays.nbytes)
        d_rays.write(rays)
        hits = {m: DevBuf(hip, n * 32) for m in METHODS}
        bits = {m: DevBuf(hip, 4 * ((n + 31) // 32)) for m in METHODS}
        ran, count = {}, {}

        # The timed calls pass stats = NULL, as a caller that wants the answers does: the statistics cost each wave
        # an atomic per counter on one cache line, a term that is the same for every method and would hide
        # what the traversals differ in.  --stats times the calls with statistics instead.
        def occluded(m):
            ctx.occluded_into(d_rays.ptr, n, bits[m].ptr, m, with_stats=args.stats)

        def intersect(m):
            ctx.intersect_into(d_rays.ptr, n, hits[m].ptr, m, with_stats=args.stats)

        calls = {}
        for m in METHODS:
            st = ctx.occluded_into(d_rays.ptr, n, bits[m].ptr, m, with_stats=True)  # (untimed: what ran, the count)
            ran[m], count[m] = st.method_ran, st.occluded
            calls[("occluded", m)] = lambda m=m: occluded(m)
            calls[("intersect", m)] = lambda m=m: intersect(m)
        ms = measure(calls, args.repeat)
        kind = hits[_lib.QUERY_SCAN].read().view(np.uint32).reshape(-1, 8)[:, 1]
        want = np.packbits(kind != 0, bitorder="little")
        for m in METHODS:
            got = bits[m].read()[:len(want)]
            if not np.array_equal(got, want):
                raise RuntimeError(f"{workload}: {_lib.QUERY_NAMES[m]} bits differ from kind != 0 of scan's hits")
        for m in METHODS:
            o, i = ms[("occluded", m)], ms[("intersect", m)]
            mo, mi = statistics.median(o), statistics.median(i)
            rec = {"tool": "occlusion_rate", "tag": args.tag, "build_id": _lib.build_id(), "scene": args.scene,
                   "workload": workload, "with_stats": bool(args.stats), "size": [W, H], "rays": n, "occluded_rays": int(count[m]),
                   "method": _lib.QUERY_NAMES[m], "method_ran": _lib.QUERY_NAMES[ran[m]], "calls": len(o),
                   "occluded_ms_median": round(mo, 4), "occluded_ms_min": round(min(o), 4),
                   "occluded_ms_max": round(max(o), 4), "intersect_ms_median": round(mi, 4),
                   "intersect_ms_min": round(min(i), 4), "intersect_ms_max": round(max(i), 4),
                   "occluded_mrays_per_s": round(n / mo / 1e3, 2), "intersect_mrays_per_s": round(n / mi / 1e3, 2),
                   "occluded_speedup": round(mi / mo, 3), "bvh_built": info["bvh_built"], "triangles": len(pipe.tris)}
            lines.append(rec)
            print(json.dumps(rec))
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
