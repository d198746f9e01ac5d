#!/usr/bin/env python3
"""The CPU grid the guided upsample's default footprint was chosen from: tests/upsample_ref.py on the
CPU oracle's frames of box and spheres.  The low image is 1, 4 or 16 frames traced and accumulated at 64 x 64, 1 spp,
8 bounces, RGBA32F; the guides are the first hits of the 64 x 64 view and of the target-size view of the same camera;
the targets are 128 x 128 and 160 x 160 (a ratio that is not an integer); the error is the mean squared error of the
rgb against the oracle's accumulation of 256 frames of other offsets traced at the target size.  Four reconstructions:
  (a) the nearest rule, what hrt_present does today;
  (b) the guided upsample, footprint 2;
  (c) the guided upsample, footprint 4;
  (d) footprint 2 after the variance-guided denoise (tests/variance_ref.py, defaults) of the low image.
Prints one JSON line per scene, target size and frame count, then which of (b) and (c) is lower on both scenes.
Usage: python tools/upsample_grid.py"""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pyoracle  # noqa: E402
import upsample_ref as U  # noqa: E402
import variance_ref as V  # noqa: E402
from helpers import SceneCase  # noqa: E402

F32 = np.float32
LOW = (64, 64)
TARGETS = ((128, 128), (160, 160))
FRAMES = (1, 4, 16)
TARGET_FRAMES, TARGET_OFFSET = 256, 5000


@functools.lru_cache(maxsize=None)
def view(name, size):
    """(case, first hits) of a scene at a size."""
    from test_history_ref import first_hits
    case = SceneCase(name, size, num_samples=1, max_bounces=8)
    return case, first_hits(case)


@functools.lru_cache(maxsize=None)
def target(name, size):
    case, _ = view(name, size)
    acc = np.zeros(size[::-1] + (4,), F32)
    for k in range(TARGET_FRAMES):
        pyoracle.accumulate_rgba32f(k, acc, case.oracle(rng_offset=TARGET_OFFSET + k, want_f32=True)[1])
    return acc


@functools.lru_cache(maxsize=None)
def low_state(name, frames):
    """(accumulator, counts, moments) of the first `frames` frames at the low size."""
    case, _ = view(name, LOW)
    h, w = LOW[::-1]
    acc, cnt, mom = np.zeros((h, w, 4), F32), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    for k in range(frames):
        acc, cnt, mom = V.accumulate_history_moments(acc, cnt, mom, case.oracle(rng_offset=1 + k, want_f32=True)[1], 1 << 24)
    return acc, cnt, mom


def mse(img, ref):
    return float(np.mean((img[..., :3].astype(np.float64) - ref[..., :3]) ** 2))


def main():
    wins = {2: 0, 4: 0}
    lower_on = {2: set(), 4: set()}
    for name in ("box", "spheres"):
        _, lo = view(name, LOW)
        for size in TARGETS:
            _, hi = view(name, size)
            ref = target(name, size)
            for frames in FRAMES:
                acc, cnt, mom = low_state(name, frames)
                filtered, _ = V.denoise_variance(acc, cnt, mom, 5, V.DEFAULTS, lo)
                rec = {"scene": name, "target": list(size), "frames": frames,
                       "a_nearest": mse(U.nearest_upsample(acc, *size), ref),
                       "b_footprint2": mse(U.upsample(acc, lo, hi, 2), ref),
                       "c_footprint4": mse(U.upsample(acc, lo, hi, 4), ref),
                       "d_variance_footprint2": mse(U.upsample(filtered, lo, hi, 2), ref)}
                best = 2 if rec["b_footprint2"] <= rec["c_footprint4"] else 4
                wins[best] += 1
                lower_on[best].add(name)
                print(json.dumps(rec), flush=True)
    both = [fp for fp in (2, 4) if not lower_on[6 - fp]]
    print(json.dumps({"lower_error_points": {str(k): v for k, v in wins.items()},
                      "lower_on_every_point_of_both_scenes": both[0] if both else None}), flush=True)


if __name__ == "__main__":
    main()
