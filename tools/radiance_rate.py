#!/usr/bin/env python3
"""Radiance-query rates (hrt_radiance), per scene:

  frame   every pixel of the view as a query (origin cam_pos, seed rng_offset * 719393 + id, centre id) at the
          frame's own samples and bounces, by BVH and PAIRS (and SCAN with --frame-scan), against hrt_trace of
          the same frame on the same context (an RGBA32F context: the trace image is compared with the queries'
          output before anything is reported);
  probe   N surface-origin probe queries (origin on a random triangle pushed off along its normal, random unit
          centre, random seed) at --probe-samples and the same bounces, by SCAN, BVH and PAIRS.

Queries and results live in device memory and the timed calls pass stats = NULL.  Per workload the calls take
turns: two warm-up calls each, then `--repeat` timed rounds in which every call runs once.  hrt_radiance is
blocking; hrt_trace is timed with the hrt_synchronize that follows it.  One JSON line per (workload, call):
median / min / max milliseconds, Mqueries/s and Msegments/s from the median, and the ratio to the workload's
baseline (hrt_trace for `frame`, PAIRS for `probe`).

    python tools/radiance_rate.py --scene island --size 1920 1080 --out profiles/radiance_rate.jsonl"""
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
from query_rate import METHODS, DevBuf, measure  # noqa: E402


def probe_queries(tris, n, seed, offset):
    rng = np.random.default_rng([seed, 3])
    idx = rng.integers(0, len(tris), n)
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
    e1, e2 = tris["edge_one"][idx, :3].astype(np.float64), tris["edge_two"][idx, :3].astype(np.float64)
    p = tris["a"][idx, :3] + u[:, None] * e1 + v[:, None] * e2
    nrm = np.cross(e1, e2)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    c = rng.normal(size=(n, 3))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return E.HrtContext.radiance_queries(p + offset * nrm, rng.integers(0, 1 << 32, n), c)


def same(a, b):
    a, b = a.view(np.float32), b.view(np.float32)
    return not ((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).any()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="island")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--probes", type=int, default=1_000_000)
    ap.add_argument("--probe-samples", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frame-scan", action="store_true", help="time SCAN on the frame workload too (slow)")
    ap.add_argument("--tag", default="product")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()

    hip = ctypes.CDLL("libamdhip64.so")
    camera, settings = E.preset(args.scene)
    settings.num_samples, settings.max_bounces = args.samples, args.bounces
    W, H = args.size
    ctx = E.HrtContext((W, H), device=args.device, mode=_lib.MODE_RGBA32F)
    pipe = E.RayTracePipeline(ctx, (W, H), settings)
    info = ctx.scene_info()
    lines = []

    def report(workload, n, samples, ms, baseline, segments, ran):
        base = statistics.median(ms[baseline])
        for name, t in ms.items():
            med = statistics.median(t)
            rec = {"tool": "radiance_rate", "tag": args.tag, "build_id": _lib.build_id(), "scene": args.scene,
                   "workload": workload, "size": [W, H], "queries": n, "samples": samples, "bounces": args.bounces,
                   "segments": int(segments), "call": name, "method_ran": ran.get(name), "calls": len(t),
                   "ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                   "mqueries_per_s": round(n / med / 1e3, 3), "msegments_per_s": round(segments / med / 1e3, 2),
                   "baseline": baseline, "times_baseline": round(med / base, 3), "bvh_built": info["bvh_built"],
                   "triangles": len(pipe.tris)}
            lines.append(rec)
            print(json.dumps(rec), flush=True)

    # ---- frame ----
    frame = 1
    pc = pipe.push_constants(camera, frame, False)
    ids = np.arange(W * H)
    queries = pipe.pixel_queries(camera, ids % W, ids // W, frame)
    n = len(queries)
    d_q = DevBuf(hip, queries.nbytes)
    d_q.write(queries)
    methods = METHODS if args.frame_scan else METHODS[1:]
    out = {m: DevBuf(hip, n * 16) for m in methods}
    ran = {}
    segments = 0
    for m in methods:
        st = ctx.radiance_into(pc, d_q.ptr, n, out[m].ptr, m, with_stats=True)  # (untimed: what ran, the count)
        ran[_lib.QUERY_NAMES[m]], segments = _lib.QUERY_NAMES[st.method_ran], st.segments

    def trace():
        ctx.trace(pc)
        ctx.lib.hrt_synchronize(ctx.handle)

    calls = {"hrt_trace": trace}
    for m in methods:
        calls[_lib.QUERY_NAMES[m]] = lambda m=m: ctx.radiance_into(pc, d_q.ptr, n, out[m].ptr, m)
    ms = measure(calls, args.repeat)
    image = ctx.read(_lib.IMG_TRACE, _lib.FMT_RGBA32F).reshape(-1)
    for m in methods:
        if not same(out[m].read(), image):
            raise RuntimeError(f"frame: {_lib.QUERY_NAMES[m]} differs from the traced image")
    report("frame", n, args.samples, ms, "hrt_trace", segments, ran)

    # ---- probe ----
    diag = float(np.linalg.norm(pipe.tris["a"][:, :3].max(0) - pipe.tris["a"][:, :3].min(0)))
    probes = probe_queries(pipe.tris, args.probes, args.seed, 1e-3 * diag)
    ppc = pipe.push_constants(camera, 0, False)
    ppc.num_samples = args.probe_samples
    n = len(probes)
    d_p = DevBuf(hip, probes.nbytes)
    d_p.write(probes)
    pout = {m: DevBuf(hip, n * 16) for m in METHODS}
    ran = {}
    for m in METHODS:
        st = ctx.radiance_into(ppc, d_p.ptr, n, pout[m].ptr, m, with_stats=True)
        ran[_lib.QUERY_NAMES[m]], segments = _lib.QUERY_NAMES[st.method_ran], st.segments
    ms = measure({_lib.QUERY_NAMES[m]: (lambda m=m: ctx.radiance_into(ppc, d_p.ptr, n, pout[m].ptr, m)) for m in METHODS},
                 args.repeat)
    want = pout[_lib.QUERY_SCAN].read()
    for m in METHODS[1:]:
        if not same(pout[m].read(), want):
            raise RuntimeError(f"probe: {_lib.QUERY_NAMES[m]} differs from scan")
    report("probe", n, args.probe_samples, ms, "pairs", segments, ran)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
