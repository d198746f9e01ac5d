#!/usr/bin/env python3
"""What the guided upsample costs (hrt_upsample_present): island and cave, RGBA8 contexts, at
960x540 -> 1920x1080 and 1920x1080 -> 3840x2160.  The low context folds four 1-spp frames with per-pixel counts and
moments (so that the variance-guided filter has its inputs); its own first hits and those of a second context of the
target's size under the same camera are written once by hrt_first_hits; everything is in device memory.

Per scene and size, two warm-up rounds, then five timed rounds; a round is one call of every variant, each followed
by hrt_synchronize and timed to its return, the variants taking turns:

  present        hrt_present of the accumulator into the same target (the nearest filter: what a caller has today)
  up2 / up4      hrt_upsample_present, footprint 2 / 4, no filter
  up2v / up4v    the same with the variance-guided filter first (defaults)
  variance       hrt_denoise_variance_present into a target of the low size (what the filter alone costs)

Reported per variant: median, minimum and maximum ms per call.  One JSON line per scene and size, appended to --out
(default profiles/upsample_rate.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("island", "cave")
SIZES = (((960, 540), (1920, 1080)), ((1920, 1080), (3840, 2160)))
WARMUP, CALLS, MAX_HISTORY = 2, 5, 32


def three(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def measure(scene, low_size, high_size):
    import torch

    import epq_raytracer_amd as E
    from epq_raytracer_amd import _lib

    (ws, hs), (wt, ht) = low_size, high_size
    camera, settings = E.preset(scene)
    settings.num_samples, settings.max_bounces = 1, 8
    low = E.HrtContext(low_size, device=0, mode=_lib.MODE_RGBA8)
    high = E.HrtContext(high_size, device=0, mode=_lib.MODE_RGBA8)
    raytrace, diffuse = E.RayTracePipeline(low, low_size, settings), E.DiffusePipeline(low, low_size)
    guide_rt = E.RayTracePipeline(high, high_size, settings)
    for frame in range(4):
        raytrace.compute(camera, frame)
        diffuse.next_frame_history(raytrace.image(), MAX_HISTORY, moments=True)
    lo = torch.empty((hs * ws, 8), dtype=torch.float32, device="cuda:0")  # hrt_hit records
    hi = torch.empty((ht * wt, 8), dtype=torch.float32, device="cuda:0")
    raytrace.first_hits_async(camera, lo.data_ptr())
    guide_rt.first_hits_async(camera, hi.data_ptr())
    low.order_after(high)
    target = torch.empty((ht, wt, 4), dtype=torch.uint8, device="cuda:0")
    small = torch.empty((hs, ws, 4), dtype=torch.uint8, device="cuda:0")
    vinfo = low.variance_info()

    def up(footprint, variance):
        return lambda: low.upsample_present(target.data_ptr(), target.numel(), wt, ht, lo.data_ptr(), hi.data_ptr(),
                                            variance=variance, footprint=footprint)

    variants = {
        "present": lambda: low.present(_lib.IMG_ACCUM, target.data_ptr(), target.numel(), wt, ht),
        "up2": up(2, None), "up4": up(4, None), "up2v": up(2, vinfo), "up4v": up(4, vinfo),
        "variance": lambda: low.denoise_variance_present(small.data_ptr(), small.numel(), ws, hs, guide_ptr=lo.data_ptr()),
    }
    ms = {name: [] for name in variants}
    low.synchronize()
    high.synchronize()
    for rnd in range(WARMUP + CALLS):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            low.synchronize()
            if rnd >= WARMUP:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    # what the guided forms change: the share of target pixels that differ from the nearest filter's
    variants["present"]()
    low.synchronize()
    nearest = target.clone()
    variants["up2"]()
    low.synchronize()
    differs = round(float((target != nearest).any(-1).float().mean()), 4)
    rec = {"scene": scene, "low": [ws, hs], "target": [wt, ht], "mode": "rgba8", "calls": CALLS, "warmup": WARMUP,
           "build_id": _lib.build_id(), "ms_per_call": {name: three(v) for name, v in ms.items()},
           "up2_pixels_differing_from_present": differs}
    low.close()
    high.close()
    return rec


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_rate.jsonl"))
    ap.add_argument("--scenes", nargs="*", default=list(SCENES))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for scene in a.scenes:
        for low_size, high_size in SIZES:
            line = json.dumps(measure(scene, low_size, high_size))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
