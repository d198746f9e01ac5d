#!/usr/bin/env python3
"""What fold records and hrt_compute_until cost the headline loop: island 1920x1080, 64 spp, 8 bounces,
64-frame launches; per-frame wall time (ms) of

  p  hrt_compute_n on another build of the library (--baseline-lib, the parent commit's)
  a  hrt_compute_n, HRT_OPT_FOLD_RECORDS off         (the same launches as p)
  b  hrt_compute_n, HRT_OPT_FOLD_RECORDS on          (the recording combiner)
  c  hrt_compute_until with a rule that cannot be met (trace, count pass, host read, fold: every launch)

each in a fresh process (one warm-up launch of 64 frames, then --calls timed launches), the variants
interleaved, --rounds times.  Every child runs under its own time limit and the first failing one ends the
run.  One JSON line per child, then a summary line (median per variant, p's spread, differences to p).

    python tools/fold_records_cost.py --baseline-lib PATH [--rounds 5] [--calls 3] [--out profiles/fold_records.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

SCENE, SIZE, SPP, BOUNCES, BATCH = "island", (1920, 1080), 64, 8, 64


def child(variant: str, calls: int) -> dict:
    from helpers import SceneCase, _lib

    case = SceneCase(SCENE, SIZE, SPP, BOUNCES)
    options = {_lib.OPT_FRAMES_PER_LAUNCH: BATCH}
    if variant == "b":
        options[_lib.OPT_FOLD_RECORDS] = 1
    ctx = case.context(options=options)
    ctx.trace(case.push(init=True))
    ctx.accumulate(0)

    def run(first):
        if variant == "c":
            # (a quiet run longer than the call: never met, whatever the frames hold -- at this size and sample
            # count whole frames fold without changing a pixel from about frame 70 on)
            done, settled = ctx.compute_until(case.push(first), BATCH, max_changed_pixels=0, max_delta=0,
                                              quiet_frames=BATCH + 1)
            assert (done, settled) == (BATCH, False), (done, settled)
        else:
            ctx.compute_n(case.push(first), BATCH)
        ctx.synchronize()

    run(1)  # warm-up: the frame stack, the plan, the tile lists
    ms = []
    for k in range(calls):
        t0 = time.perf_counter()
        run(1 + BATCH * (k + 1))
        ms.append(round((time.perf_counter() - t0) * 1e3 / BATCH, 4))
    out = {"variant": variant, "ms_per_frame": ms, "build_id": _lib.build_id()}
    if variant == "b":
        recs, total = ctx.fold_records(with_total=True)
        out["records"] = int(total)
        out["last_changed_pixels"] = int(recs[-1]["changed_pixels"])
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.calls)))
        return
    variants = (["p"] if a.baseline_lib else []) + ["a", "b", "c"]
    lines = []
    for r in range(a.rounds):
        for v in variants:
            env = dict(os.environ)
            if v == "p":
                env["HRT_LIB"] = os.path.abspath(a.baseline_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "a" if v == "p" else v,
                                "--calls", str(a.calls)], env=env, capture_output=True, text=True, timeout=180)
            if p.returncode != 0:
                print(json.dumps({"variant": v, "round": r, "error": p.stderr[-2000:], "rc": p.returncode}))
                sys.exit(1)
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            rec.update(variant=v, round=r)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    med = {v: statistics.median(x for ln in lines if ln["variant"] == v for x in ln["ms_per_frame"]) for v in variants}
    summary = {"summary": True, "scene": SCENE, "size": list(SIZE), "spp": SPP, "bounces": BOUNCES, "batch": BATCH,
               "rounds": a.rounds, "calls": a.calls, "median_ms_per_frame": {v: round(m, 4) for v, m in med.items()},
               "build_id": next(ln["build_id"] for ln in lines if ln["variant"] == "a")}
    if "p" in med:
        pv = [x for ln in lines if ln["variant"] == "p" for x in ln["ms_per_frame"]]
        summary["baseline_build_id"] = next(ln["build_id"] for ln in lines if ln["variant"] == "p")
        summary["baseline_spread_ms"] = [min(pv), max(pv)]
        summary["minus_baseline_ms_per_64_frames"] = {v: round((med[v] - med["p"]) * BATCH, 3) for v in "abc"}
    print(json.dumps(summary))
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines + [summary]:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
