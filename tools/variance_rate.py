#!/usr/bin/env python3
"""What the variance-guided denoise costs (hrt_denoise_variance and the moments calls): island
1920x1080, RGBA8 context, four 1-spp frames folded with per-pixel counts and moments, a small camera move carried
across by hrt_reproject_moments and one more frame folded (so that both variance estimates run), the new view's
first hits as the guide, everything in device memory.

The filter: two warm-up rounds, then five timed rounds; a round is one blocking call of every variant at every
iteration count 0..5, the variants taking turns -- DIRECT, TILED and AUTO of hrt_denoise_variance, and hrt_denoise
AUTO on the same accumulator (iterations 1..5).  Every method's image and variance are compared with DIRECT's before
anything is reported.  Reported per variant: median, minimum and maximum ms per call by iteration count, and per step
the same three of the per-round differences of consecutive iteration counts (iterations 0 is variance_prep, the
store and the call's fixed cost).  auto_per_step names, per step, TILED where it runs a kernel of its own (steps 1, 2
and 4) and its maximum is below DIRECT's minimum (the ranges are apart), else DIRECT.

The history calls: hrt_accumulate_history_moments against hrt_accumulate_history and hrt_reproject_moments against
hrt_reproject, each call followed by hrt_synchronize, taking turns, two warm-ups and five timed calls each.

One JSON line, appended to --out (default profiles/variance_rate.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE, SIZE, WARMUP, CALLS = "island", (1920, 1080), 2, 5
MAX_HISTORY = 32


def three(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance_rate.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import epq_raytracer_amd as E
    from epq_raytracer_amd import _lib

    W, H = SIZE
    camera, settings = E.preset(SCENE)
    settings.num_samples, settings.max_bounces = 1, 8
    ctx = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
    raytrace, diffuse = E.RayTracePipeline(ctx, SIZE, settings), E.DiffusePipeline(ctx, SIZE)
    for frame in range(4):
        raytrace.compute(camera, frame)
        diffuse.next_frame_history(raytrace.image(), MAX_HISTORY, moments=True)
    d0 = np.asarray(camera.direction, np.float64) / np.linalg.norm(camera.direction)
    side = np.cross(d0, np.asarray(camera.up, np.float64))
    side /= np.linalg.norm(side)
    moved = E.Camera([float(c + 0.01 * s) for c, s in zip(camera.position, side)],
                     [float(v) for v in d0 + (3.0 / H) * side], camera.up)
    guides = [torch.empty((H * W, 8), dtype=torch.float32, device="cuda:0") for _ in range(2)]  # hrt_hit records
    raytrace.first_hits_into(camera, guides[0].data_ptr())
    raytrace.first_hits_into(moved, guides[1].data_ptr())
    views = [E.View(camera, SIZE, settings), E.View(moved, SIZE, settings)]
    ctx.reproject_moments(views[0], guides[0].data_ptr(), views[1], guides[1].data_ptr())
    raytrace.compute(moved, 4)
    diffuse.next_frame_history(raytrace.image(), MAX_HISTORY, moments=True)
    counts = ctx.read_history()
    guide = guides[1].data_ptr()

    # ---- the filter ----
    methods = {"direct": _lib.VARIANCE_DIRECT, "tiled": _lib.VARIANCE_TILED, "auto": _lib.VARIANCE_AUTO}
    variants = list(methods) + ["hrt_denoise_auto"]
    outs = {m: torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0") for m in variants}
    vars_ = {m: torch.empty((H, W), dtype=torch.float32, device="cuda:0") for m in methods}
    nbytes = W * H * 4
    its = list(range(0, _lib.VARIANCE_MAX_ITERATIONS + 1))
    vinfos = {(m, k): ctx.variance_info(iterations=k, method=v) for m, v in methods.items() for k in its}
    dinfos = {k: ctx.denoise_info(iterations=k, method=_lib.DENOISE_AUTO) for k in its if k}

    def call(m, k):
        if m == "hrt_denoise_auto":
            ctx.denoise_into(outs[m].data_ptr(), nbytes, _lib.FMT_RGBA8, guide, dinfos[k])
        else:
            ctx.denoise_variance_into(outs[m].data_ptr(), nbytes, _lib.FMT_RGBA8, guide, vars_[m].data_ptr(), nbytes,
                                      vinfos[(m, k)])

    ms = {(m, k): [] for m in variants for k in its if k or m != "hrt_denoise_auto"}
    for rnd in range(WARMUP + CALLS):
        for k in its:
            for m in variants:
                if (m, k) not in ms:
                    continue
                t0 = time.perf_counter()
                call(m, k)
                if rnd >= WARMUP:
                    ms[(m, k)].append((time.perf_counter() - t0) * 1e3)
            if rnd == 0:
                for m in methods:
                    same_v = torch.equal(vars_[m].view(torch.int32), vars_["direct"].view(torch.int32))
                    if not torch.equal(outs[m], outs["direct"]) or not same_v:
                        print(f"{m} differs from direct at {k} iterations", file=sys.stderr)
                        return 1
    rec = {"scene": SCENE, "width": W, "height": H, "guided": True, "mode": "rgba8", "fmt": "rgba8", "calls": CALLS,
           "warmup": WARMUP, "build_id": _lib.build_id(),
           "pixels_below_min_history": round(float((counts < _lib.VARIANCE_MIN_HISTORY).mean()), 4), "variants": {}}
    steps = {}
    for m in variants:
        ks = [k for k in its if (m, k) in ms]
        per_call = {str(k): three(ms[(m, k)]) for k in ks}
        step = {}
        for k in ks[1:]:  # per round: this iteration count less the one before
            step[str(1 << (k - 1))] = three([x - y for x, y in zip(ms[(m, k)], ms[(m, k - 1)])]) if (m, k - 1) in ms else None
        steps[m] = step
        rec["variants"][m] = {"ms_per_call_by_iterations": per_call, "ms_per_step": step}
    # (at steps 8 and 16 TILED runs the direct kernel: what the two variants differ by there is the noise of the method)
    rec["auto_per_step"] = {s: ("tiled" if int(s) <= 4 and steps["tiled"][s]["max"] < steps["direct"][s]["min"] else "direct")
                            for s in steps["direct"]}
    full = str(_lib.VARIANCE_MAX_ITERATIONS)
    rec["auto_over_hrt_denoise_auto"] = round(rec["variants"]["auto"]["ms_per_call_by_iterations"][full]["median"] /
                                              rec["variants"]["hrt_denoise_auto"]["ms_per_call_by_iterations"][full]["median"], 4)

    # ---- the history calls ----
    def timed(fn):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    pairs = {
        "accumulate_history": lambda: ctx.accumulate_history(MAX_HISTORY),
        "accumulate_history_moments": lambda: ctx.accumulate_history_moments(MAX_HISTORY),
        "reproject": lambda: ctx.reproject(views[0], guides[0].data_ptr(), views[1], guides[1].data_ptr()),
        "reproject_moments": lambda: ctx.reproject_moments(views[0], guides[0].data_ptr(), views[1], guides[1].data_ptr()),
    }
    hist = {name: [] for name in pairs}
    ctx.synchronize()
    for rnd in range(WARMUP + CALLS):
        for name, fn in pairs.items():
            t = timed(fn)
            if rnd >= WARMUP:
                hist[name].append(t)
    rec["history_calls_ms"] = {name: three(v) for name, v in hist.items()}
    ctx.close()
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
