#!/usr/bin/env python3
"""What the denoise pass costs (hrt_denoise): island 1920x1080, RGBA8 context, three 1-spp
frames accumulated, the view's first hits as the guide, everything in device memory.  For each method and each
iteration count 1..5: two warm-up calls, then five timed blocking calls; the methods take turns (one timed call
each per round), and every method's output is compared with DIRECT's before anything is reported.

Reported per method: the median ms per call at 1..5 iterations, and per step the difference of consecutive
medians (step 1 also carries denoise_prep and the call's fixed cost).  A guided pass moves at least 52 bytes
per pixel (16 colour in, 16 guide, 4 key, 16 out): that compulsory traffic over the step's time, as a fraction
of the HBM peak (8 TB/s), is reported beside it.  best_per_step names, per step, the faster of DIRECT and TILED.
--forms also times the debug library's two forms of the tiled kernel at every step (dense tile: steps 1, 2, 4;
sub-lattice: every step).  One JSON line, appended to --out (default profiles/denoise_rate.jsonl).
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
HBM_PEAK = 8.0e12  # bytes / s
STEP_BYTES = 52    # per pixel, guided


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_rate.jsonl"))
    ap.add_argument("--forms", action="store_true", help="also the debug library's dense and sub-lattice forms")
    a = ap.parse_args()
    import torch

    import epq_raytracer_amd as E
    from epq_raytracer_amd import _lib

    W, H = SIZE
    camera, settings = E.preset(SCENE)
    settings.num_samples, settings.max_bounces = 1, 8
    ctx = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8, debug=a.forms)
    raytrace, diffuse = E.RayTracePipeline(ctx, SIZE, settings), E.DiffusePipeline(ctx, SIZE)
    for frame in range(4):
        raytrace.compute(camera, frame)
        diffuse.next_frame(frame, raytrace.image())
    guide = torch.empty((H * W, 8), dtype=torch.float32, device="cuda:0")
    raytrace.first_hits_into(camera, guide.data_ptr())
    methods = {"direct": _lib.DENOISE_DIRECT, "tiled": _lib.DENOISE_TILED, "auto": _lib.DENOISE_AUTO}
    if a.forms:
        methods.update(dense=_lib.DEBUG_DENOISE_DENSE, lattice=_lib.DEBUG_DENOISE_LATTICE)
    outs = {m: torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0") for m in methods}
    nbytes = W * H * 4
    ms = {m: [] for m in methods}
    for iterations in range(1, _lib.DENOISE_MAX_ITERATIONS + 1):
        infos = {m: ctx.denoise_info(iterations=iterations, method=v) for m, v in methods.items()}
        for _ in range(WARMUP):
            for m in methods:
                ctx.denoise_into(outs[m].data_ptr(), nbytes, _lib.FMT_RGBA8, guide.data_ptr(), infos[m])
        for m in methods:
            if not torch.equal(outs[m], outs["direct"]):
                print(f"{m} differs from direct at {iterations} iterations", file=sys.stderr)
                return 1
        runs = {m: [] for m in methods}
        for _ in range(CALLS):
            for m in methods:
                t0 = time.perf_counter()
                ctx.denoise_into(outs[m].data_ptr(), nbytes, _lib.FMT_RGBA8, guide.data_ptr(), infos[m])
                runs[m].append((time.perf_counter() - t0) * 1e3)
        for m in methods:
            ms[m].append(statistics.median(runs[m]))
    rec = {"scene": SCENE, "width": W, "height": H, "guided": True, "mode": "rgba8", "fmt": "rgba8", "calls": CALLS,
           "warmup": WARMUP, "build_id": _lib.build_id(), "debug_library": bool(a.forms), "methods": {}}
    steps = {}
    for m in methods:
        step = [ms[m][0]] + [ms[m][k] - ms[m][k - 1] for k in range(1, len(ms[m]))]
        steps[m] = step
        rec["methods"][m] = {
            "ms_per_call_by_iterations": [round(v, 4) for v in ms[m]],
            "ms_per_step": [round(v, 4) for v in step],  # step 1 includes denoise_prep and the call's fixed cost
            "compulsory_fraction_of_hbm_peak": [round(W * H * STEP_BYTES / (max(v, 1e-6) * 1e-3) / HBM_PEAK, 4) for v in step]}
    rec["best_per_step"] = ["tiled" if steps["tiled"][k] < steps["direct"][k] else "direct" for k in range(len(steps["direct"]))]
    ctx.close()
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
