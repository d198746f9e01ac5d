#!/usr/bin/env python3
"""How a progressive render settles: the fold record of every frame (HRT_OPT_FOLD_RECORDS) and the frame at
which a settle rule would stop hrt_compute_until.

    python tools/settle_curve.py [--scene island --size 96x64 --spp 3 --bounces 8 --frames 24]
                                 [--max-changed N] [--max-delta N] [--quiet-frames N] [--mode rgba8|rgba32f]

From a cleared accumulator, frames 1..frames through hrt_compute_n with the option on; one JSON line per
frame (frame, changed_pixels, abs_delta_sum, max_delta), then one line with the rule, the stop frame it
gives on those records, and what hrt_compute_until itself returns for the same rule on a fresh context."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import fold_ref  # noqa: E402
from helpers import SceneCase, _lib  # noqa: E402


def cleared_context(case, mode, records):
    ctx = case.context(mode=mode, options={_lib.OPT_FOLD_RECORDS: int(records)})
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="island")
    ap.add_argument("--size", default="96x64")
    ap.add_argument("--spp", type=int, default=3)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--mode", choices=("rgba8", "rgba32f"), default="rgba8")
    ap.add_argument("--max-changed", type=int, default=fold_ref.ANY)
    ap.add_argument("--max-delta", type=int, default=fold_ref.ANY)
    ap.add_argument("--quiet-frames", type=int, default=1)
    a = ap.parse_args()
    if not 0 < a.frames < _lib.FOLD_RECORD_RING:
        ap.error(f"--frames must be in [1, {_lib.FOLD_RECORD_RING - 1}]: the ring keeps that many records")
    size = tuple(int(v) for v in a.size.split("x"))
    mode = _lib.MODE_RGBA8 if a.mode == "rgba8" else _lib.MODE_RGBA32F
    case = SceneCase(a.scene, size, a.spp, a.bounces)
    ctx = cleared_context(case, mode, True)
    ctx.compute_n(case.push(1), a.frames)
    recs = ctx.fold_records()[-a.frames:]
    ctx.close()
    rows = []
    for r in recs:
        rows.append((int(r["changed_pixels"]), int(r["abs_delta_sum"]), int(r["max_delta"])))
        print(json.dumps({"frame": int(r["frame"]), "changed_pixels": rows[-1][0], "abs_delta_sum": rows[-1][1],
                          "max_delta": rows[-1][2]}))
    stop, settled = fold_ref.stop_frame(rows, a.frames, a.max_changed, a.max_delta, a.quiet_frames)
    ctx = cleared_context(case, mode, False)
    done, ok = ctx.compute_until(case.push(1), a.frames, a.max_changed, a.max_delta, a.quiet_frames)
    ctx.close()
    print(json.dumps({"scene": a.scene, "size": a.size, "spp": a.spp, "bounces": a.bounces, "mode": a.mode,
                      "rule": {"max_changed_pixels": a.max_changed, "max_delta": a.max_delta,
                               "quiet_frames": a.quiet_frames},
                      "stop_frame": stop, "settled": settled, "compute_until": {"frames_done": done, "settled": ok},
                      "build_id": _lib.build_id()}))


if __name__ == "__main__":
    main()
