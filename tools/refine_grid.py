#!/usr/bin/env python3
"""The CPU grid the adaptive refinement's defaults were chosen from: tests/refine_ref.py's chain on
the CPU oracle's frames of box and spheres at 64 x 64, 1 spp, 8 bounces, RGBA32F, guide = the view's first hits, error
against the oracle's accumulation of 1,024 frames of other offsets.  Prints one JSON line per grid point with the
three conditions tests/test_refine_ref.py holds the defaults to:
  (a) spheres, 64 passes: MSE below the uniform curve's at ceil(pixel_frames / npix) frames;
  (b) spheres, 64 passes: pixel_frames at most half of 64 npix;
  (c) box, 32 passes: at least 85 % of the pixels selected by the 32nd pass, and MSE at most 1.1 x the uniform
      curve's at floor(pixel_frames / npix) frames.
Usage: python tools/refine_grid.py [--floor 0.01]"""
import argparse
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import history_ref as H  # noqa: E402
import pyoracle  # noqa: E402
import refine_ref as R  # noqa: E402
from helpers import SceneCase  # noqa: E402

F32 = np.float32
SIZE = (64, 64)
TARGET_FRAMES, TARGET_OFFSET = 1024, 5000


@functools.lru_cache(maxsize=None)
def scene(name):
    """(frame(k), target, surface keys) of a scene: frame(k) is the oracle's RGBA32F frame at rng_offset 1 + k."""
    from test_history_ref import first_hits
    case = SceneCase(name, SIZE, num_samples=1, max_bounces=8)
    target = np.zeros(SIZE[::-1] + (4,), F32)
    for k in range(TARGET_FRAMES):
        pyoracle.accumulate_rgba32f(k, target, case.oracle(rng_offset=TARGET_OFFSET + k, want_f32=True)[1])
    frame = functools.lru_cache(maxsize=None)(lambda k: case.oracle(rng_offset=1 + k, want_f32=True)[1])
    return frame, target, R.keys_of(first_hits(case), SIZE[::-1])


def mse(acc, target):
    return float(np.mean((acc[..., :3].astype(np.float64) - target[..., :3]) ** 2))


def uniform_mse(name, frames: int):
    """The same frames folded for every pixel."""
    frame, target, _ = scene(name)
    acc, cnt = np.zeros_like(target), np.zeros(SIZE[::-1], np.uint32)
    for k in range(frames):
        acc, cnt = H.accumulate_history(acc, cnt, frame(k), 1 << 24)
    return mse(acc, target)


def adaptive(name, passes: int, rule):
    """(MSE, pixel_frames, selected per pass) of the chain from an empty history."""
    frame, target, key = scene(name)
    h, w = SIZE[::-1]
    acc, cnt, mom = np.zeros_like(target), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32)
    acc, cnt, mom, _, pf, _, counts = R.refine_until(acc, cnt, mom, frame, 1 << 24, passes, key, rule)
    return mse(acc, target), pf, counts


def conditions(rule):
    npix = SIZE[0] * SIZE[1]
    s_mse, s_pf, _ = adaptive("spheres", 64, rule)
    s_uni = uniform_mse("spheres", -(-s_pf // npix))
    b_mse, b_pf, b_counts = adaptive("box", 32, rule)
    b_uni = uniform_mse("box", b_pf // npix)
    share = (b_counts[31] if len(b_counts) >= 32 else 0) / npix
    return {
        "spheres": {"mse": s_mse, "frames": s_pf / npix, "uniform_mse": s_uni},
        "box": {"mse": b_mse, "frames": b_pf / npix, "uniform_mse": b_uni, "selected_share_pass32": share},
        "a": s_mse < s_uni, "b": s_pf <= 32 * npix, "c": share >= 0.85 and b_mse <= 1.1 * b_uni,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--floor", type=float, default=R.DEFAULTS[4])
    args = ap.parse_args()
    for mh in (4, 8):
        for radius in (0, 1, 3):
            for tol in (0.02, 0.05, 0.1, 0.2):
                rule = (mh, 1 << 24, radius, tol, args.floor)
                print(json.dumps({"min_history": mh, "radius": radius, "tolerance": tol, "floor": args.floor,
                                  **conditions(rule)}), flush=True)


if __name__ == "__main__":
    main()
