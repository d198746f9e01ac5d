#!/usr/bin/env python3
"""What temporal upsampling buys on the CPU: tests/resolve_ref.py on the CPU oracle's frames of box
and spheres.  The low grid is 64 x 64, 1 spp, 8 bounces, RGBA32F; the targets are 128 x 128 and 160 x 160 (a ratio
that is not an integer); the error is the mean squared error of the rgb against the oracle's accumulation of 256
frames of other offsets traced at the target size.  For 4, 16 and 64 low frames, three pictures:
  (a) hrt_upsample, footprint 2, of the plain low accumulation of as many frames (the low grid where it is, its own
      default jitter): what a caller has today;
  (b) the resolved history: frame k traced on the low grid shifted by hrt_history_phase(k), jitter_size the target
      grid's default jitter, folded by hrt_accumulate_history_from (unguided, FILL, MOMENTS, no history cap);
  (c) (b) behind the variance-guided denoise (tests/variance_ref.py, defaults, guided by the target's first hits).
Prints one JSON line per scene, target size and frame count, then the points at which (b) and (c) are lower than (a).
Usage: python tools/resolve_grid.py"""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import epq_raytracer_amd as E  # noqa: E402
import history_ref as H  # noqa: E402
import resolve_ref as R  # noqa: E402
import upsample_ref as U  # noqa: E402
import variance_ref as V  # noqa: E402
from epq_raytracer_amd import _lib  # noqa: E402
from helpers import SceneCase  # noqa: E402

F32 = np.float32
LOW = (64, 64)
TARGETS = ((128, 128), (160, 160))
FRAMES = (4, 16, 64)
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
    # (hrt_accumulate_history's fold from an empty history: the mean of all 256 frames -- the reference's combiner
    # clears on frame 0, so 256 calls of it would hold 255 frames over 256)
    acc, cnt = np.zeros(size[::-1] + (4,), F32), np.zeros(size[::-1], np.uint32)
    for k in range(TARGET_FRAMES):
        acc, cnt = H.accumulate_history(acc, cnt, case.oracle(rng_offset=TARGET_OFFSET + k, want_f32=True)[1], 1 << 24)
    return acc


def shifted_case(name, size, offset):
    """The low case with its ray grid shifted by offset pixels and the target grid's default jitter."""
    case = SceneCase(name, LOW, num_samples=1, max_bounces=8)
    s = case.settings
    first, dx, dy, _ = E.ray_grid(LOW, s.camera_focal_length, s.viewport_height, s.up)
    first = E.shifted_first(first, dx, dy, *offset)
    ys, xs = np.mgrid[0:LOW[1], 0:LOW[0]]
    fx, fy = xs.astype(F32)[..., None], ys.astype(F32)[..., None]
    c = ((first + dx * fx).astype(F32) + (dy * fy).astype(F32)).astype(F32)
    rays = np.zeros(LOW[0] * LOW[1], dtype=_lib.RAY_DTYPE)
    rays["sample_centre"][:, :3] = c.reshape(-1, 3)
    rays["sample_centre"][:, 3] = 1.0
    case.rays = rays
    case.jitter = float(np.float32(E.ray_grid(size, s.camera_focal_length, s.viewport_height, s.up)[3]))
    return case


def low_states(name):
    """frames -> the plain low accumulator after that many frames."""
    case, _ = view(name, LOW)
    acc, cnt, out = np.zeros(LOW[::-1] + (4,), F32), np.zeros(LOW[::-1], np.uint32), {}
    for k in range(max(FRAMES)):
        acc, cnt = H.accumulate_history(acc, cnt, case.oracle(rng_offset=1 + k, want_f32=True)[1], 1 << 24)
        if k + 1 in FRAMES:
            out[k + 1] = acc
    return out


def resolved_states(name, size):
    """frames -> (A, N, M) of the target-size history after that many shifted low frames."""
    w, h = size
    nx, ny = R.phases(LOW[0], w), R.phases(LOW[1], h)
    cases = {}
    state = (np.zeros((h, w, 4), F32), np.zeros((h, w), np.uint32), np.zeros((h, w, 2), F32))
    out = {}
    for k in range(max(FRAMES)):
        off = R.history_phase(LOW[0], w, LOW[1], h, k)
        key = k % (nx * ny)
        if key not in cases:
            cases[key] = shifted_case(name, size, off)
        tex = cases[key].oracle(rng_offset=1 + k, want_f32=True)[1]
        state = R.resolve(*state, tex, off, 1 << 24, R.FILL | R.MOMENTS)[:3]
        if k + 1 in FRAMES:
            out[k + 1] = state
    return out


def mse(img, ref):
    return float(np.mean((img[..., :3].astype(np.float64) - ref[..., :3]) ** 2))


def main():
    b_lower, c_lower, points = [], [], 0
    for name in ("box", "spheres"):
        _, lo = view(name, LOW)
        plain = low_states(name)
        for size in TARGETS:
            _, hi = view(name, size)
            ref = target(name, size)
            resolved = resolved_states(name, size)
            for frames in FRAMES:
                acc, cnt, mom = resolved[frames]
                filtered, _ = V.denoise_variance(acc, cnt, mom, 5, V.DEFAULTS, hi)
                rec = {"scene": name, "target": list(size), "frames": frames,
                       "a_upsample_footprint2": mse(U.upsample(plain[frames], lo, hi, 2), ref),
                       "b_resolved": mse(acc, ref), "c_resolved_variance": mse(filtered, ref),
                       "min_count": int(cnt.min()), "max_count": int(cnt.max())}
                points += 1
                tag = f"{name} {size[0]} {frames}"
                if rec["b_resolved"] < rec["a_upsample_footprint2"]:
                    b_lower.append(tag)
                if rec["c_resolved_variance"] < rec["a_upsample_footprint2"]:
                    c_lower.append(tag)
                print(json.dumps(rec), flush=True)
    print(json.dumps({"points": points, "b_lower_than_a": b_lower, "c_lower_than_a": c_lower}), flush=True)


if __name__ == "__main__":
    main()
