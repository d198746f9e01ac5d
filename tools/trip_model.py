#!/usr/bin/env python3
"""Lane-schedule model of trace_fused_split's loop: a Monte Carlo run of one wave's 64 lanes
under the two thresholds, costed with the per-phase shader clocks of the diagnostics kernel.  CPU only; it
is a model, not a measurement.

    python3 tools/trip_model.py [--record profiles/phase_batch_step0.jsonl] [--scene island] [--segments 2000000]

The wave: 64 lanes that are always refilled (the pixel pool).  A ready lane's primary segment hits with
probability --p-hit; a hit survives the roulette with --p-live and the lane then waits for a bounce batch; a
bounce segment hits with --p-bounce-hit, survives the same way, and a path ends at --bounces segments after
the first.  Per trip, as the kernel: run_sec = W > 0 and (W >= sec or R == 0); run_prim = R > 0 and (not
run_sec or R >= prim).

The costs come from the record: for every (prim_batch, sec_batch) row the diagnostics kernel counted the
primary trips, batches and fused trips and summed the clocks of the three phases, whose lane totals do not
depend on the thresholds.  A least-squares line per phase over the rows -- clocks = fixed x trips + rest --
gives the fixed cost of a primary phase, of a batch and of a trip's shading; `rest` is the lane-proportional
part.  The model's trips and batches per segment times those fixed costs, plus the rests, is its predicted
clock sum per row, printed beside the measured one (both relative to the row (1, 28), or --base).  The
first row of a scene in the record is its context's first, unplanned trace and is left out of the fit."""
import argparse
import json
import random


def simulate(prim, sec, a, rng):
    """(primary trips, batches, fused trips, primary lanes, bounce lanes) for a.segments segments."""
    bounce = [0] * 64  # 0: ready; k > 0: waiting for the path's segment k
    pt = bt = trips = pl = bl = 0
    while pl + bl < a.segments:
        ready = [i for i in range(64) if bounce[i] == 0]
        wait = [i for i in range(64) if bounce[i] != 0]
        R, W = len(ready), len(wait)
        run_sec = W > 0 and (W >= sec or R == 0)
        run_prim = R > 0 and (not run_sec or R >= prim)
        trips += 1
        if run_prim:
            pt += 1
            pl += R
            for i in ready:
                live = rng.random() < a.p_hit and rng.random() < a.p_live and a.bounces > 0
                bounce[i] = 1 if live else 0
        if run_sec:
            bt += 1
            bl += W
            for i in wait:
                live = rng.random() < a.p_bounce_hit and rng.random() < a.p_live and bounce[i] < a.bounces
                bounce[i] = bounce[i] + 1 if live else 0
    return pt, bt, trips, pl, bl


def fit(xs, ys):
    """Least squares y = k x + c."""
    n = len(xs)
    mx, my = sum(xs) / n, sum(ys) / n
    sxx = sum((x - mx) ** 2 for x in xs)
    k = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sxx if sxx else 0.0
    return k, my - k * mx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", default="profiles/phase_batch_step0.jsonl")
    ap.add_argument("--scene", default="island")
    ap.add_argument("--segments", type=int, default=2000000)
    ap.add_argument("--p-hit", type=float, default=0.93)
    ap.add_argument("--p-live", type=float, default=0.552)
    ap.add_argument("--p-bounce-hit", type=float, default=0.18)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--base", default="1,28")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rows = [json.loads(l) for l in open(a.record) if l.startswith("{")]
    rows = [r for r in rows if r.get("scene") == a.scene and r.get("lib") == "new"]
    fitted = rows[1:]  # (the context's first trace is unplanned)
    kp, cp = fit([r["fused_primary_iters"] for r in fitted], [r["primary_cycles"] for r in fitted])
    kb, cb = fit([r["bounce_iters"] for r in fitted], [r["bounce_cycles"] for r in fitted])
    ks, cs = fit([r["loop_iters"] for r in fitted], [r["shade_cycles"] for r in fitted])
    lanes = rows[0]["primary_lanes"] + rows[0]["bounce_lanes"]
    print(json.dumps({"scene": a.scene, "fit": "clocks = fixed x trips + rest, per phase, over the record's rows",
                      "primary_phase_fixed": round(kp), "batch_fixed": round(kb), "shading_per_trip": round(ks),
                      "rest_per_lane": round((cp + cb + cs) / lanes, 1)}))
    out = {}
    for r in rows:
        pb, sb = r["prim_batch"], r["sec_batch"]
        pt, bt, trips, pl, bl = simulate(pb, sb, a, random.Random(a.seed))
        seg = pl + bl
        model = (kp * pt + kb * bt + ks * trips) / seg + (cp + cb + cs) / lanes
        meas = (r["primary_cycles"] + r["bounce_cycles"] + r["shade_cycles"]) / lanes
        out[(pb, sb)] = dict(prim_batch=pb, sec_batch=sb, model_primary_fill=round(pl / max(pt, 1), 1),
                             model_batch_fill=round(bl / max(bt, 1), 1),
                             measured_primary_fill=round(r["primary_lanes"] / max(r["fused_primary_iters"], 1), 1),
                             measured_batch_fill=round(r["bounce_lanes"] / max(r["bounce_iters"], 1), 1),
                             model_clocks_per_segment=model, measured_clocks_per_segment=meas)
    base = out[tuple(int(v) for v in a.base.split(","))]["model_clocks_per_segment"]
    for rec in out.values():
        rec["model_vs_base"] = round(rec.pop("model_clocks_per_segment") / base, 4)
        rec["measured_clocks_per_segment"] = round(rec["measured_clocks_per_segment"], 1)
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
