#!/usr/bin/env python3
"""What the fold across resolutions costs (hrt_accumulate_history_from): island, both modes, at
960x540 -> 1920x1080 and 1920x1080 -> 3840x2160.  The low context traces one 1-spp frame; its first hits and those
of the target-size context under the same camera are written once by hrt_first_hits; the target-size context traces
one frame of its own, so that hrt_accumulate_history has a trace image to fold.  Everything is in device memory.

Per size and mode, two warm-up rounds, then five timed rounds; a round is one call of every variant, each followed by
hrt_synchronize and timed to its return, the variants taking turns, the offset that of the round's phase:

  history        hrt_accumulate_history on the target-size context (the same-size fold: what a caller has today)
  from           hrt_accumulate_history_from, unguided, FILL
  from_m         ... with MOMENTS
  from_g         ... guided by the two first-hit arrays
  from_gm        ... guided, with MOMENTS
  set_ray_grid   hrt_set_ray_grid on the low context

Reported per variant: median, minimum and maximum ms per call.  One JSON line per size and mode, appended to --out
(default profiles/resolve_rate.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE = "island"
SIZES = (((960, 540), (1920, 1080)), ((1920, 1080), (3840, 2160)))
WARMUP, CALLS, MAX_HISTORY = 2, 5, 32


def three(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def measure(low_size, high_size, mode_name):
    import torch

    import epq_raytracer_amd as E
    from epq_raytracer_amd import _lib

    (ws, hs), (w, h) = low_size, high_size
    mode = _lib.MODE_RGBA8 if mode_name == "rgba8" else _lib.MODE_RGBA32F
    camera, settings = E.preset(SCENE)
    settings.num_samples, settings.max_bounces = 1, 8
    low = E.HrtContext(low_size, device=0, mode=mode)
    high = E.HrtContext(high_size, device=0, mode=mode)
    low_rt, high_rt = E.RayTracePipeline(low, low_size, settings), E.RayTracePipeline(high, high_size, settings)
    lo = torch.empty((hs * ws, 8), dtype=torch.float32, device="cuda:0")  # hrt_hit records
    hi = torch.empty((h * w, 8), dtype=torch.float32, device="cuda:0")
    low_rt.first_hits_async(camera, lo.data_ptr())
    high_rt.first_hits_async(camera, hi.data_ptr())
    low_rt.compute(camera, 1)
    high_rt.compute(camera, 1)
    phase = [0]

    def offset():
        return E.history_phase(low_size, high_size, phase[0])

    def fold(moments, guided):
        return lambda: high.accumulate_history_from(low, offset(), MAX_HISTORY, moments=moments,
                                                    source_hits_ptr=lo.data_ptr() if guided else None,
                                                    hits_ptr=hi.data_ptr() if guided else None)

    variants = {
        "history": (high, lambda: high.accumulate_history(MAX_HISTORY)),
        "from": (high, fold(False, False)), "from_m": (high, fold(True, False)),
        "from_g": (high, fold(False, True)), "from_gm": (high, fold(True, True)),
        "set_ray_grid": (low, lambda: low_rt.shift_rays(*offset())),
    }
    ms = {name: [] for name in variants}
    low.synchronize()
    high.synchronize()
    for rnd in range(WARMUP + CALLS):
        phase[0] = rnd
        for name, (waited, fn) in variants.items():
            t0 = time.perf_counter()
            fn()
            waited.synchronize()
            if rnd >= WARMUP:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    counts = high.read_history()
    rec = {"scene": SCENE, "low": [ws, hs], "target": [w, h], "mode": mode_name, "calls": CALLS, "warmup": WARMUP,
           "build_id": _lib.build_id(), "ms_per_call": {name: three(v) for name, v in ms.items()},
           "min_count_after": int(counts.min())}
    low.close()
    high.close()
    return rec


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resolve_rate.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for low_size, high_size in SIZES:
        for mode_name in ("rgba8", "rgba32f"):
            line = json.dumps(measure(low_size, high_size, mode_name))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
