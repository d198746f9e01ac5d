#!/usr/bin/env python3
"""What adaptive refinement costs (hrt_refine_select, hrt_refine, hrt_refine_until): island and cave
1920x1080, 64 spp, 8 bounces, RGBA8 context, everything in device memory.

Pass cost by share.  Four history frames with moments, the view's first hits, the default rule's selection; that mask
is dilated (4-neighbourhood) until it covers a target share and thinned by a per-pixel hash down to it, for shares of
about 1, 5, 10, 25, 50 and 100 %.  One blocking hrt_refine pass per (share, method), QUERIES and FRAME taking turns:
one warm-up round, then five timed rounds; median, minimum and maximum ms.  crossover = the smallest share from which
FRAME's maximum is below QUERIES' minimum (the ranges apart) at every larger share too; null when there is none.

Selection cost.  hrt_refine_select alone into a device mask with the count read back, guided and not, two warm-ups and
five timed calls.

End to end.  The four history frames, then hrt_refine_until with the defaults (at most 256 passes), against
hrt_compute_until with the documented rule (no changed pixel in a fold, at most 256 frames, after the cleared image
folded as frame 0) on a second context: wall time, passes or frames, pixel_frames / npix, and the mean absolute
difference (8-bit steps, rgb) of both accumulators from the mean of 256 frames of other offsets.

One JSON line per scene, appended to --out (default profiles/refine_rate.jsonl).

--tiles: the tile-masked passes instead (hrt_refine_tiles, hrt_refine_tiles_until; run_tiles below), one
JSON line per scene appended to profiles/refine_tiles_rate.jsonl.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, SPP, BOUNCES, WARMUP, CALLS = (1920, 1080), 64, 8, 1, 5
SHARES = (0.01, 0.05, 0.10, 0.25, 0.50, 1.0)
HISTORY = 1 << 24


def three(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def mask_at_share(sel, share):
    """sel dilated until it covers `share` of the image, then thinned by a hash of the pixel index down to it."""
    import numpy as np
    h, w = sel.shape
    if share >= 1.0:
        return np.ones((h, w), bool)
    cur = sel.copy()
    if not cur.any():
        cur[h // 2, w // 2] = True
    while cur.mean() < share:
        grown = cur.copy()
        grown[1:] |= cur[:-1]
        grown[:-1] |= cur[1:]
        grown[:, 1:] |= cur[:, :-1]
        grown[:, :-1] |= cur[:, 1:]
        cur = grown
    i = np.arange(h * w, dtype=np.uint64).reshape(h, w)
    u = ((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 2.0**32
    return cur & (u < share / cur.mean())


def run(scene, out_path):
    import numpy as np
    import torch

    import epq_raytracer_amd as E
    from epq_raytracer_amd import _lib

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refine_ref as R

    W, H = SIZE
    npix = W * H
    camera, settings = E.preset(scene)
    settings.num_samples, settings.max_bounces = SPP, BOUNCES

    def history_context():
        ctx = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
        raytrace, diffuse = E.RayTracePipeline(ctx, SIZE, settings), E.DiffusePipeline(ctx, SIZE)
        for frame in range(_lib.REFINE_MIN_HISTORY):
            raytrace.compute(camera, frame)
            diffuse.next_frame_history(raytrace.image(), HISTORY, moments=True)
        return ctx, raytrace, diffuse

    ctx, raytrace, diffuse = history_context()
    guide = torch.empty((npix, 8), dtype=torch.float32, device="cuda:0")  # hrt_hit records
    raytrace.first_hits_async(camera, guide.data_ptr())
    words = ctx.mask_words
    dmask = torch.zeros(words, dtype=torch.int32, device="cuda:0")
    rec = {"scene": scene, "width": W, "height": H, "spp": SPP, "bounces": BOUNCES, "mode": "rgba8", "calls": CALLS,
           "warmup": WARMUP, "build_id": _lib.build_id()}

    # ---- selection cost ----
    sel_ms = {"guided": [], "unguided": []}
    for rnd in range(2 + CALLS):
        for name, ptr in (("guided", guide.data_ptr()), ("unguided", None)):
            t0 = time.perf_counter()
            n = ctx.refine_select_into(dmask.data_ptr(), ptr, True)
            if rnd >= 2:
                sel_ms[name].append((time.perf_counter() - t0) * 1e3)
    n = ctx.refine_select_into(dmask.data_ptr(), guide.data_ptr(), True)
    rec["select_ms"] = {k: three(v) for k, v in sel_ms.items()}
    rec["selected_share_after_history"] = round(n / npix, 4)
    real = R.unpack_mask(dmask.cpu().numpy().view(np.uint32), (H, W))

    # ---- pass cost by share ----
    masks = {}
    for share in SHARES:
        m = mask_at_share(real, share)
        masks[share] = (torch.from_numpy(R.pack_mask(m).view(np.int32)).to("cuda:0"), float(m.mean()))
    methods = {"queries": _lib.REFINE_QUERIES, "frame": _lib.REFINE_FRAME}
    ms = {(s, m): [] for s in SHARES for m in methods}
    offset = 100
    for rnd in range(WARMUP + CALLS):
        for share in SHARES:
            for m, method in methods.items():
                pc = raytrace.push_constants(camera, offset, False)
                offset += 1
                t0 = time.perf_counter()
                ctx.refine(pc, masks[share][0].data_ptr(), HISTORY, method, 0, True, want_stats=False)
                if rnd >= WARMUP:
                    ms[(share, m)].append((time.perf_counter() - t0) * 1e3)
    rec["pass_ms_by_share"] = {f"{masks[s][1]:.4f}": {m: three(ms[(s, m)]) for m in methods} for s in SHARES}
    frame_wins = [max(ms[(s, "frame")]) < min(ms[(s, "queries")]) for s in SHARES]
    queries_wins = [max(ms[(s, "queries")]) < min(ms[(s, "frame")]) for s in SHARES]
    cross = None
    for k, s in enumerate(SHARES):
        if all(frame_wins[k:]) and all(queries_wins[:k]):
            cross = round(masks[s][1], 4)
            break
    rec["crossover_share"] = cross
    rec["winner_by_share"] = ["frame" if f else "queries" if q else "overlap" for f, q in zip(frame_wins, queries_wins)]
    ctx.close()

    # ---- end to end ----
    # (hrt_compute_n ties the combiner's frame number to the rng offset, so the reference of other offsets is folded
    # with per-pixel counts: the plain mean of its 256 frames, in the context's 8-bit arithmetic)
    ref = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
    rpipe, rdiff = E.RayTracePipeline(ref, SIZE, settings), E.DiffusePipeline(ref, SIZE)
    for k in range(256):
        rpipe.compute(camera, 5000 + k)
        rdiff.next_frame_history(rpipe.image(), HISTORY)
    target = ref.read(_lib.IMG_ACCUM)[..., :3].astype(np.float64)
    ref.close()

    t0 = time.perf_counter()
    ctx, raytrace, diffuse = history_context()
    raytrace.first_hits_async(camera, guide.data_ptr())
    t1 = time.perf_counter()
    passes, pixel_frames, settled = diffuse.refine_until(raytrace, camera, _lib.REFINE_MIN_HISTORY, 256, HISTORY,
                                                         guide.data_ptr())
    t2 = time.perf_counter()
    acc = ctx.read(_lib.IMG_ACCUM)[..., :3].astype(np.float64)
    counts = ctx.read_history()
    ctx.close()
    rec["refine_until"] = {"history_ms": round((t1 - t0) * 1e3, 3), "refine_ms": round((t2 - t1) * 1e3, 3), "passes": passes,
                           "settled": settled, "pixel_frames_over_npix": round(pixel_frames / npix, 4),
                           "frames_per_pixel_mean": round(float(counts.mean()), 4), "frames_per_pixel_max": int(counts.max()),
                           "mean_abs_diff": round(float(np.abs(acc - target).mean()), 4)}
    ctx = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
    cpipe = E.RayTracePipeline(ctx, SIZE, settings)
    # the reference application's loop: the cleared image folded as frame 0, then the frames 1, 2, ...
    t0 = time.perf_counter()
    cpipe.init()
    ctx.accumulate(0)
    frames, settled = ctx.compute_until(cpipe.push_constants(camera, 1, False), 256, max_changed_pixels=0)
    t1 = time.perf_counter()
    acc = ctx.read(_lib.IMG_ACCUM)[..., :3].astype(np.float64)
    ctx.close()
    rec["compute_until"] = {"ms": round((t1 - t0) * 1e3, 3), "frames": frames, "settled": settled,
                            "image_mean": round(float(acc.mean()), 3), "reference_mean": round(float(target.mean()), 3),
                            "mean_abs_diff": round(float(np.abs(acc - target).mean()), 4)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


TILE_FRAMES = (1, 4, 16)


def run_tiles(scene, out_path):
    """--tiles: the tile-masked passes (hrt_refine_tiles) beside hrt_refine(FRAME), same workload and
    masks.  Per share: tiles_selected / tiles, and one blocking pass of FRAME and of hrt_refine_tiles at 1, 4 and 16
    frames taking turns (ms per frame; one warm-up round, five timed).  End to end: hrt_refine_until(FRAME),
    hrt_refine_tiles_until at 1 and 4 frames per pass and hrt_compute_until, each from a fresh context."""
    import numpy as np
    import torch

    import epq_raytracer_amd as E
    from epq_raytracer_amd import _lib

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refine_ref as R

    W, H = SIZE
    npix = W * H
    camera, settings = E.preset(scene)
    settings.num_samples, settings.max_bounces = SPP, BOUNCES

    def history_context():
        ctx = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
        raytrace, diffuse = E.RayTracePipeline(ctx, SIZE, settings), E.DiffusePipeline(ctx, SIZE)
        for frame in range(_lib.REFINE_MIN_HISTORY):
            raytrace.compute(camera, frame)
            diffuse.next_frame_history(raytrace.image(), HISTORY, moments=True)
        return ctx, raytrace, diffuse

    ctx, raytrace, diffuse = history_context()
    guide = torch.empty((npix, 8), dtype=torch.float32, device="cuda:0")  # hrt_hit records
    raytrace.first_hits_async(camera, guide.data_ptr())
    dmask = torch.zeros(ctx.mask_words, dtype=torch.int32, device="cuda:0")
    rec = {"scene": scene, "width": W, "height": H, "spp": SPP, "bounces": BOUNCES, "mode": "rgba8", "calls": CALLS,
           "warmup": WARMUP, "build_id": _lib.build_id()}
    ctx.refine_select_into(dmask.data_ptr(), guide.data_ptr(), True)
    real = R.unpack_mask(dmask.cpu().numpy().view(np.uint32), (H, W))

    # ---- pass cost by share ----
    masks = {}
    for share in SHARES:
        m = mask_at_share(real, share)
        masks[share] = (torch.from_numpy(R.pack_mask(m).view(np.int32)).to("cuda:0"), float(m.mean()))
    variants = ["frame"] + [f"tiles_{f}" for f in TILE_FRAMES]
    ms = {(s, v): [] for s in SHARES for v in variants}
    tile_share, kernels = {}, set()
    offset = 100
    for rnd in range(WARMUP + CALLS):
        for share in SHARES:
            for v in variants:
                frames = 1 if v == "frame" else int(v.split("_")[1])
                pc = raytrace.push_constants(camera, offset, False)
                offset += frames
                t0 = time.perf_counter()
                if v == "frame":
                    ctx.refine(pc, masks[share][0].data_ptr(), HISTORY, _lib.REFINE_FRAME, 0, True, want_stats=False)
                else:
                    st = ctx.refine_tiles(pc, masks[share][0].data_ptr(), HISTORY, frames)
                dt = (time.perf_counter() - t0) * 1e3 / frames
                if v != "frame":
                    tile_share[share] = (st.tiles_selected / st.tiles, st.whole_frame, st.items)
                    kernels.add(_lib.KERNEL_NAMES.get(st.kernel_ran, str(st.kernel_ran)))
                if rnd >= WARMUP:
                    ms[(share, v)].append(dt)
    rec["kernel"] = sorted(kernels)
    rec["pass_ms_per_frame_by_share"] = {
        f"{masks[s][1]:.4f}": dict({v: three(ms[(s, v)]) for v in variants}, tiles_selected_share=round(tile_share[s][0], 4),
                                   whole_frame=tile_share[s][1], items=tile_share[s][2]) for s in SHARES}
    # per share and frame count: tiles ahead with the ranges apart, frame ahead with the ranges apart, or overlap
    rec["tiles_against_frame"] = {
        f"{masks[s][1]:.4f}": {v: "tiles" if max(ms[(s, v)]) < min(ms[(s, "frame")]) else
                               "frame" if max(ms[(s, "frame")]) < min(ms[(s, v)]) else "overlap" for v in variants[1:]}
        for s in SHARES}
    ctx.close()

    # ---- end to end ----
    ref = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
    rpipe, rdiff = E.RayTracePipeline(ref, SIZE, settings), E.DiffusePipeline(ref, SIZE)
    for k in range(256):
        rpipe.compute(camera, 5000 + k)
        rdiff.next_frame_history(rpipe.image(), HISTORY)
    target = ref.read(_lib.IMG_ACCUM)[..., :3].astype(np.float64)
    ref.close()

    def until(name, call):
        t0 = time.perf_counter()
        ctx, raytrace, diffuse = history_context()
        raytrace.first_hits_async(camera, guide.data_ptr())
        t1 = time.perf_counter()
        passes, pixel_frames, settled = call(raytrace, diffuse)
        t2 = time.perf_counter()
        acc = ctx.read(_lib.IMG_ACCUM)[..., :3].astype(np.float64)
        counts = ctx.read_history()
        ctx.close()
        rec[name] = {"history_ms": round((t1 - t0) * 1e3, 3), "refine_ms": round((t2 - t1) * 1e3, 3), "passes": passes,
                     "settled": settled, "pixel_frames_over_npix": round(pixel_frames / npix, 4),
                     "frames_per_pixel_mean": round(float(counts.mean()), 4), "frames_per_pixel_max": int(counts.max()),
                     "mean_abs_diff": round(float(np.abs(acc - target).mean()), 4)}

    first = _lib.REFINE_MIN_HISTORY
    until("refine_until_frame", lambda rt, df: df.refine_until(rt, camera, first, 256, HISTORY, guide.data_ptr(), _lib.REFINE_FRAME))
    until("refine_tiles_until_1", lambda rt, df: df.refine_tiles_until(rt, camera, first, 256, 1, HISTORY, guide.data_ptr()))
    until("refine_tiles_until_4", lambda rt, df: df.refine_tiles_until(rt, camera, first, 64, 4, HISTORY, guide.data_ptr()))
    ctx = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
    cpipe = E.RayTracePipeline(ctx, SIZE, settings)
    t0 = time.perf_counter()
    cpipe.init()
    ctx.accumulate(0)
    frames, settled = ctx.compute_until(cpipe.push_constants(camera, 1, False), 256, max_changed_pixels=0)
    t1 = time.perf_counter()
    acc = ctx.read(_lib.IMG_ACCUM)[..., :3].astype(np.float64)
    ctx.close()
    rec["compute_until"] = {"ms": round((t1 - t0) * 1e3, 3), "frames": frames, "settled": settled,
                            "mean_abs_diff": round(float(np.abs(acc - target).mean()), 4)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="default profiles/refine_rate.jsonl, with --tiles profiles/refine_tiles_rate.jsonl")
    ap.add_argument("--scenes", default="island,cave")
    ap.add_argument("--tiles", action="store_true", help="the tile-masked passes beside FRAME (run_tiles)")
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", "refine_tiles_rate.jsonl" if a.tiles else "refine_rate.jsonl")
    for scene in a.scenes.split(","):
        (run_tiles if a.tiles else run)(scene, out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
