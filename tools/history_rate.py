#!/usr/bin/env python3
"""What the temporal history costs (hrt_reproject, hrt_accumulate_history): island 1920x1080, both
context modes, everything in device memory.  Per mode: a context with a few frames of history, the first hits
of the base view, of a small move (a turn of two pixels and a short step) and of a large one (a turn of a
fifth of the image) written by hrt_intersect_primary into device buffers.  Variants, taking turns (one timed
call each per round), two warm-up rounds, then five timed ones, each call timed to hrt_synchronize:

  reproject_{nearest,bilinear}_{small,large}   hrt_reproject from the base view to the moved one (every count
                                               refilled to 8 before the call, outside the timing, so that each
                                               call sees the same history)
  fold_history                                 hrt_accumulate_history(32) of the newest trace image
  accumulate                                   hrt_accumulate of the same images (the parent's fold)

Reported per variant: the median ms, the compulsory bytes per pixel -- reproject: the pixel's own hit record and
one source record, texel and count in, texel and count out (80 B in RGBA8 mode, 104 B in RGBA32F); fold:
accumulator in and out, trace texel and count in, count out (20 / 56 B; hrt_accumulate: 12 / 48) -- and that
traffic over the time as a fraction of the HBM peak (8 TB/s); fold_history / accumulate as a ratio, and the
share of pixels each move keeps.  One JSON line per mode, appended to --out (default
profiles/history_rate.jsonl).

--motion: what the motion forms cost beside the plain ones (hrt_reproject_motion[_moments]): island
and cave at 1920x1080, both modes, the small move, BILINEAR.  Variants, taking turns in the same way (two warm-up
rounds, five timed calls each, timed to hrt_synchronize, the host copy of the tables included):

  plain, plain_moments               hrt_reproject, hrt_reproject_moments
  one_mesh, one_mesh_moments         the motion forms with mesh 0 moving by about two pixels, the others static
  all, all_moments                   ... with every mesh moving

The scene itself stays where it is: the pass reads the same hit records either way, and its cost does not depend on
whether the tables tell the truth.  One JSON line per scene and mode ("tool": "history_rate --motion").
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE, SIZE, WARMUP, CALLS = "island", (1920, 1080), 2, 5
HBM_PEAK = 8.0e12  # bytes / s
BYTES = {"rgba8": {"reproject": 80, "fold_history": 20, "accumulate": 12},
         "rgba32f": {"reproject": 104, "fold_history": 56, "accumulate": 48}}


def turned(E, cam, dpos, turn):
    d = np.asarray(cam.direction, np.float64)
    d /= np.linalg.norm(d)
    up = np.asarray(cam.up, np.float64)
    side = np.cross(d, up)
    side /= np.linalg.norm(side)
    nd = d + turn[0] * side + turn[1] * up
    return E.Camera([float(a + b) for a, b in zip(cam.position, dpos)], [float(v) for v in nd], cam.up)


def motion_rates(E, _lib, torch):
    """--motion: one record per scene and mode."""
    W, H = SIZE
    px = 2.0 / H
    lines = []
    for scene in ("island", "cave"):
        for mode_name, mode in (("rgba8", _lib.MODE_RGBA8), ("rgba32f", _lib.MODE_RGBA32F)):
            camera, settings = E.preset(scene)
            settings.num_samples, settings.max_bounces = 1, 8
            ctx = E.HrtContext(SIZE, device=0, mode=mode)
            raytrace, diffuse = E.RayTracePipeline(ctx, SIZE, settings), E.DiffusePipeline(ctx, SIZE)
            for frame in range(4):
                raytrace.compute(camera, frame)
                diffuse.next_frame_history(raytrace.image(), moments=True)
            cams = {"base": camera, "small": turned(E, camera, (0.02, 0.0, 0.01), (2 * px, -px))}
            views = {k: E.View(c, SIZE, settings) for k, c in cams.items()}
            hits = {k: torch.empty((H * W, 8), dtype=torch.float32, device="cuda:0") for k in cams}
            for k, c in cams.items():
                raytrace.first_hits_into(c, hits[k].data_ptr())
            info = ctx.reproject_info(filter=_lib.REPROJECT_BILINEAR)
            n = len(settings.mesh_data)
            depth = float(np.linalg.norm(np.asarray(camera.position, np.float64)))  # the scenes sit around the origin
            ident = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
            moved = E.motion_between(ident, ident[:9] + [2 * px * depth, 0.0, px * depth])
            still = E.motion_between(ident, ident)
            tables = {"one_mesh": ctx.motion_tables(None, [moved] + [still] * (n - 1)),
                      "all": ctx.motion_tables(None, [moved] * n)}
            args = (views["base"], hits["base"].data_ptr(), views["small"], hits["small"].data_ptr())

            def plain(moments):
                (ctx.reproject_moments if moments else ctx.reproject)(*args, info)

            def motion(which, moments):
                ctx.reproject_motion(*args, moments=moments, info=info, tables=tables[which][0])

            variants = {"plain": lambda: plain(False), "plain_moments": lambda: plain(True)}
            for which in tables:
                variants[which] = lambda which=which: motion(which, False)
                variants[which + "_moments"] = lambda which=which: motion(which, True)
            runs = {v: [] for v in variants}
            for rnd in range(WARMUP + CALLS):
                for v, call in variants.items():
                    ctx.fill_history(8)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    call()
                    ctx.synchronize()
                    if rnd >= WARMUP:
                        runs[v].append((time.perf_counter() - t0) * 1e3)
            rec = {"tool": "history_rate --motion", "scene": scene, "width": W, "height": H, "mode": mode_name,
                   "calls": CALLS, "warmup": WARMUP, "meshes": n, "build_id": _lib.build_id(), "variants": {}}
            for v in variants:
                rec["variants"][v] = {"median_ms": round(statistics.median(runs[v]), 4), "min_ms": round(min(runs[v]), 4),
                                      "max_ms": round(max(runs[v]), 4)}
            ctx.close()
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    return lines


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_rate.jsonl"))
    ap.add_argument("--motion", action="store_true", help="the motion forms beside the plain ones (see above)")
    a = ap.parse_args()
    import torch

    import epq_raytracer_amd as E
    from epq_raytracer_amd import _lib

    if a.motion:
        lines = motion_rates(E, _lib, torch)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return 0

    W, H = SIZE
    px = 2.0 / H
    lines = []
    for mode_name, mode in (("rgba8", _lib.MODE_RGBA8), ("rgba32f", _lib.MODE_RGBA32F)):
        camera, settings = E.preset(SCENE)
        settings.num_samples, settings.max_bounces = 1, 8
        ctx = E.HrtContext(SIZE, device=0, mode=mode)
        raytrace, diffuse = E.RayTracePipeline(ctx, SIZE, settings), E.DiffusePipeline(ctx, SIZE)
        for frame in range(4):
            raytrace.compute(camera, frame)
            diffuse.next_frame_history(raytrace.image())
        cams = {"base": camera, "small": turned(E, camera, (0.02, 0.0, 0.01), (2 * px, -px)),
                "large": turned(E, camera, (0.5, 0.1, 0.2), (0.2 * W * px, 0.0))}
        views = {k: E.View(c, SIZE, settings) for k, c in cams.items()}
        hits = {k: torch.empty((H * W, 8), dtype=torch.float32, device="cuda:0") for k in cams}
        for k, c in cams.items():
            raytrace.first_hits_into(c, hits[k].data_ptr())
        infos = {"nearest": ctx.reproject_info(filter=_lib.REPROJECT_NEAREST),
                 "bilinear": ctx.reproject_info(filter=_lib.REPROJECT_BILINEAR)}
        frame_no = [4]

        def reproject(filt, move):
            ctx.reproject(views["base"], hits["base"].data_ptr(), views[move], hits[move].data_ptr(), infos[filt])

        def fold_history():
            ctx.accumulate_history(32)

        def accumulate():
            ctx.accumulate(frame_no[0])
            frame_no[0] += 1

        variants = {f"reproject_{f}_{m}": (lambda f=f, m=m: reproject(f, m)) for m in ("small", "large")
                    for f in ("nearest", "bilinear")}
        variants.update(fold_history=fold_history, accumulate=accumulate)
        runs = {v: [] for v in variants}
        kept = {}
        for rnd in range(WARMUP + CALLS):
            for v, call in variants.items():
                if v.startswith("reproject"):
                    ctx.fill_history(8)
                ctx.synchronize()
                t0 = time.perf_counter()
                call()
                ctx.synchronize()
                if rnd >= WARMUP:
                    runs[v].append((time.perf_counter() - t0) * 1e3)
                if v.startswith("reproject") and rnd == 0:
                    kept[v] = round(float((ctx.read_history() > 0).mean()), 4)
        med = {v: statistics.median(runs[v]) for v in variants}
        rec = {"scene": SCENE, "width": W, "height": H, "mode": mode_name, "calls": CALLS, "warmup": WARMUP,
               "build_id": _lib.build_id(), "variants": {}}
        for v in variants:
            b = BYTES[mode_name]["reproject" if v.startswith("reproject") else v]
            rec["variants"][v] = {"median_ms": round(med[v], 4), "min_ms": round(min(runs[v]), 4),
                                  "max_ms": round(max(runs[v]), 4), "compulsory_bytes_per_pixel": b,
                                  "compulsory_fraction_of_hbm_peak": round(W * H * b / (med[v] * 1e-3) / HBM_PEAK, 4)}
            if v in kept:
                rec["variants"][v]["pixels_kept"] = kept[v]
        rec["fold_history_over_accumulate"] = round(med["fold_history"] / med["accumulate"], 4)
        ctx.close()
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
