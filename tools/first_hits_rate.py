#!/usr/bin/env python3
"""What the first hits of a 1080p view cost (hrt_first_hits): island and cave at 1920x1080, the
hit records in device memory.  Variants, taking turns (one timed call each per round), two warm-up rounds, then
five timed ones, each call timed from before the call to the end of hrt_synchronize:

  tiles          hrt_first_hits TILES   (one wave per 8x8 tile, the tile's primary triangle list)
  query          hrt_first_hits QUERY   (hrt_intersect_primary's AUTO kernel, enqueued)
  primary_bvh    hrt_intersect_primary BVH    (blocking)
  primary_pairs  hrt_intersect_primary PAIRS  (blocking)

each for two rows: `fresh`, every call from a camera position no earlier call used (TILES rebuilds its camera
records), and `repeat`, every call from the preset's camera (TILES keeps them; nothing else differs for the
other three).  query minus primary_bvh is what the blocking form costs.  One counted TILES call per scene gives
the tile counts of the preset's view.  Per scene one JSON line with median, minimum and maximum ms per variant
and row, and whether TILES beats QUERY from a fresh camera with the five-run ranges apart (the rule AUTO
follows); written to --out (default profiles/first_hits_rate.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES, SIZE, WARMUP, CALLS = ("island", "cave"), (1920, 1080), 2, 5


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_hits_rate.jsonl"))
    a = ap.parse_args()
    import torch

    import epq_raytracer_amd as E
    from epq_raytracer_amd import _lib

    W, H = SIZE
    lines = []
    for scene in SCENES:
        camera, settings = E.preset(scene)
        ctx = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
        raytrace = E.RayTracePipeline(ctx, SIZE, settings)
        hits = torch.empty((H * W, 8), dtype=torch.float32, device="cuda:0")
        ptr = hits.data_ptr()
        moves = [0]

        def cam(fresh):
            if not fresh:
                return camera
            moves[0] += 1  # a position of its own: 1 mm steps along x
            return E.Camera([camera.position[0] + 0.001 * moves[0], *camera.position[1:]], camera.direction, camera.up)

        variants = {
            "tiles": lambda c: raytrace.first_hits_async(c, ptr, _lib.FIRST_HITS_TILES),
            "query": lambda c: raytrace.first_hits_async(c, ptr, _lib.FIRST_HITS_QUERY),
            "primary_bvh": lambda c: ctx.intersect_primary_into(raytrace.push_constants(c, 0, False), ptr, None, _lib.QUERY_BVH),
            "primary_pairs": lambda c: ctx.intersect_primary_into(raytrace.push_constants(c, 0, False), ptr, None, _lib.QUERY_PAIRS),
        }
        runs = {(v, row): [] for v in variants for row in ("fresh", "repeat")}
        raytrace.first_hits_async(camera, ptr, _lib.FIRST_HITS_TILES)  # (the repeat row's records)
        for rnd in range(WARMUP + CALLS):
            for row in ("fresh", "repeat"):
                for v, call in variants.items():
                    c = cam(row == "fresh")
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    call(c)
                    ctx.synchronize()
                    if rnd >= WARMUP:
                        runs[(v, row)].append((time.perf_counter() - t0) * 1e3)
                    if row == "fresh" and v == "tiles":  # the repeat row's TILES call finds the preset's records again
                        raytrace.first_hits_async(camera, ptr, _lib.FIRST_HITS_TILES)
        raytrace.first_hits_async(camera, ptr, _lib.FIRST_HITS_TILES, count=True)
        st = ctx.first_hits_stats()
        rec = {"scene": scene, "width": W, "height": H, "calls": CALLS, "warmup": WARMUP, "build_id": _lib.build_id(),
               "tiles": {"tiles": st.tiles, "listed": st.tiles_listed, "empty": st.tiles_empty, "fallback": st.tiles_fallback,
                         "entries_tested": st.entries_tested, "tri_tests": st.tri_tests, "scan_rays": st.scan_rays},
               "rows": {}}
        for row in ("fresh", "repeat"):
            rec["rows"][row] = {v: {"median_ms": round(statistics.median(runs[(v, row)]), 4),
                                    "min_ms": round(min(runs[(v, row)]), 4), "max_ms": round(max(runs[(v, row)]), 4)}
                                for v in variants}
        fresh = rec["rows"]["fresh"]
        rec["query_minus_primary_bvh_ms"] = round(fresh["query"]["median_ms"] - fresh["primary_bvh"]["median_ms"], 4)
        rec["tiles_over_query_fresh"] = round(fresh["tiles"]["median_ms"] / fresh["query"]["median_ms"], 4)
        rec["tiles_beats_query_ranges_apart"] = fresh["tiles"]["max_ms"] < fresh["query"]["min_ms"]
        ctx.close()
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
