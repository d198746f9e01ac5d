#!/usr/bin/env python3
"""What presenting costs the realtime loop (compute_then_render per frame, src/main.rs:41-57): island
1920x1080, 64 spp, 8 bounces, 5 warm-up frames then 32 timed frames, per-frame wall time of four variants

  a  trace + accumulate only                          (bench.py's per_frame_dispatch_ms shape)
  b  ... + a blocking hrt_read_image of the accumulator into device memory every frame
         (what a presenting user paid before hrt_present: the host waits once per frame)
  c  ... + hrt_present into device memory, waiting only for the ticket of three frames back
  d  hrt_accumulate_present (the combine and the present in one kernel), waiting as c

each in a fresh process, three times.  Usage:
    python tools/present_loop.py [--out profiles/present_loop.jsonl] [--repeats 3] [--parts N]
With --parts N > 1 the frame is rendered by N contexts of interleaved 8-row tiles, all on device 0, joined
with hrt_comm_init_all (the single-process multi-GPU layout rehearsed on one GPU: ordering and host cost,
not scaling).  Every frame traces and accumulates on every part; b reads the gathered frame with a blocking
read_frame into device memory, c presents on the group's root, d is hrt_accumulate_present on the root.
--baseline-lib PATH adds, to every repeat, variant b on another build of the library (what that build
offers a group), alternating with this build's variants.
--denoise runs two variants only, taking turns in one sitting: c, and
  e  c with hrt_denoise_present in place of hrt_present (five guided a-trous passes, default sigmas; the
     guide is the view's first hits, written once into device memory before the loop: the camera stands still)
and writes profiles/present_loop_denoise.jsonl with the ratio e / c (single context only).
--moving runs e and two variants of the temporal pipeline, taking turns in one sitting (single context only):
  f  the camera moves every frame (a sway of up to two pixels and a short step): hrt_intersect_primary of the
     new view into device memory (blocking), trace, hrt_reproject from the previous view, hrt_accumulate_history
     (max_history 32) and hrt_denoise_present guided by the new first hits
  g  f with the first hits taken on a second context of the same scene, so that the blocking query does not
     wait for the rendering context's stream
  h  f with hrt_first_hits (AUTO) into two alternating device buffers in place of the blocking call: every stage
     of the frame is enqueued, the host waits for tickets only
and writes profiles/present_loop_history.jsonl with f / e, g / e, h / e, f - g and f - h.
--variance runs two variants of the moving loop only, taking turns in one sitting: h, and
  i  h with the three moments calls in place of the plain ones: hrt_reproject_moments,
     hrt_accumulate_history_moments and hrt_denoise_variance_present (the variance-guided filter, defaults)
and writes profiles/present_loop_variance.jsonl with i / h and i - h.
--upsample runs two variants of the moving loop only, taking turns in one sitting: i, and
  j  i with the trace, the history and the filter on a context of half the size (960x540): hrt_first_hits of the
     half-size view on that context, hrt_first_hits of the full-size view on a second, full-size context of the same
     scene into two alternating buffers, hrt_order_after between the two, and hrt_upsample_present (the variance-guided
     filter first, default footprint) in place of the present
and writes profiles/present_loop_upsample.jsonl with j / i, j - i and whether the two ranges are apart.
--resolve runs three variants of the moving loop, taking turns in one sitting: i, j, and
  k  i with the trace alone on a context of half the size, its ray grid moved each frame by hrt_history_phase's
     offset (hrt_set_ray_grid, jitter_size the full-size grid's default) and the history kept at full size: on the
     full-size context hrt_first_hits, hrt_reproject_moments, hrt_accumulate_history_from (the half-size trace image
     folded into the pixels its samples landed in, with moments) and hrt_denoise_variance_present -- all enqueued
and writes profiles/present_loop_resolve.jsonl with k / i, k / j, k - j and whether k lies between j and i.
--objects runs two variants of the moving loop only, taking turns in one sitting: i, and
  m  i with one object moving as well: every frame hrt_set_scene with mesh 0 shifted (one of eight precomputed states,
     about two pixels apart), hrt_first_hits, and hrt_reproject_motion_moments with hrt_host_motion_between of the
     two states in place of hrt_reproject_moments.  hrt_set_scene rebuilds the scene and waits for the device: the
     host time spent inside it is reported separately (set_scene_ms_per_frame)
and writes profiles/present_loop_motion.jsonl with m / i, m - i and hrt_set_scene's share of m.
Every child runs under its own time limit and the first failing one ends the run.  One JSON line per
child, then a summary line (median and spread per variant, c / b and d / c).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("a", "b", "c", "d")
DENOISE_VARIANTS = ("c", "e")
MOVING_VARIANTS = ("e", "f", "g", "h")
VARIANCE_VARIANTS = ("h", "i")
UPSAMPLE_VARIANTS = ("i", "j")
RESOLVE_VARIANTS = ("i", "j", "k")
OBJECTS_VARIANTS = ("i", "m")
MAX_HISTORY = 32
SCENE, SIZE, SPP, BOUNCES, WARMUP, FRAMES, LAG = "island", (1920, 1080), 64, 8, 5, 32, 3


ROW_TILE = 8


def child(variant: str, parts: int = 1) -> dict:
    import torch

    import epq_raytracer_amd as E
    from epq_raytracer_amd import _lib

    W, H = SIZE  # the targets' size
    size = (W // 2, H // 2) if variant == "j" else SIZE  # the rendering context's
    camera, settings = E.preset(SCENE)
    settings.num_samples, settings.max_bounces = SPP, BOUNCES
    if parts > 1:
        ctxs = [E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8, partition=(ROW_TILE, p, parts))
                for p in range(parts)]
    else:
        ctxs = [E.HrtContext(size, device=0, mode=_lib.MODE_RGBA8)]
    ctx = ctxs[0]  # the root: presents, reads and holds the tickets
    raytraces = [E.RayTracePipeline(c, size, settings) for c in ctxs]
    diffuses = [E.DiffusePipeline(c, size) for c in ctxs]
    if parts > 1:
        E.HrtContext.comm_init_all(ctxs)
    targets = [torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(LAG + 1)]
    nbytes = W * H * 4
    for raytrace, diffuse in zip(raytraces, diffuses):
        raytrace.init()
        diffuse.next_frame(0, raytrace.image())
    frame, tickets = 1, []
    guide = None
    if variant == "e":
        guide = torch.empty((H * W, 8), dtype=torch.float32, device="cuda:0")  # hrt_hit records
        raytraces[0].first_hits_into(camera, guide.data_ptr())

    moving = variant in ("f", "g", "h", "i", "j", "k", "m")
    if moving:
        import numpy as np

        # first hits of the previous and the current view: LAG + 2 buffers, so that one the enqueued passes of
        # the last LAG frames still read is never overwritten
        # (h: two -- its passes are ordered on the stream behind the readers of the buffer they overwrite)
        guides = [torch.empty((size[0] * size[1], 8), dtype=torch.float32, device="cuda:0")
                  for _ in range(2 if variant in ("h", "i", "j", "k", "m") else LAG + 2)]
        guide_ctx, guide_rt = ctx, raytraces[0]
        if variant == "g":
            guide_ctx = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
            guide_rt = E.RayTracePipeline(guide_ctx, SIZE, settings)
        if variant == "j":  # the full-size view's first hits: a second context, two alternating buffers
            high_ctx = E.HrtContext(SIZE, device=0, mode=_lib.MODE_RGBA8)
            high_rt = E.RayTracePipeline(high_ctx, SIZE, settings)
            high_guides = [torch.empty((H * W, 8), dtype=torch.float32, device="cuda:0") for _ in range(2)]
            vinfo = ctx.variance_info()
        if variant == "k":  # the trace alone at half size, sampling the full-size grid's pixels phase by phase
            low_size = (W // 2, H // 2)
            low_settings = E.preset(SCENE)[1]
            low_settings.num_samples, low_settings.max_bounces = SPP, BOUNCES
            low_settings.sample_jitter = raytraces[0].sample_jitter  # the full-size grid's default jitter
            low_ctx = E.HrtContext(low_size, device=0, mode=_lib.MODE_RGBA8)
            low_rt = E.RayTracePipeline(low_ctx, low_size, low_settings)
        if variant == "m":  # eight states of the scene: mesh 0 swaying along x, records made ahead of the loop
            import copy
            states, set_scene_s = [], [0.0]
            for k in range(8):
                shift = np.array([0.15 * np.sin(2 * np.pi * k / 8), 0.0, 0.0], np.float32)
                st_settings = E.preset(SCENE)[1]
                m0 = copy.deepcopy(st_settings.mesh_data[0])
                m0.mesh.positions = (np.asarray(m0.mesh.positions, np.float32) + shift).astype(np.float32)
                st_settings.mesh_data[0] = m0
                tris, meshes = E.transform_meshes(st_settings.mesh_data)
                states.append((tris, meshes, [1, 0, 0, 0, 1, 0, 0, 0, 1] + [float(v) for v in shift]))
            still = E.motion_between(states[0][2], states[0][2])
            # (frames count from 1 and states[0] has no shift: the first frame's previous state is the preset's scene)
        d0 = np.asarray(camera.direction, np.float64) / np.linalg.norm(camera.direction)
        side = np.cross(d0, np.asarray(camera.up, np.float64))
        side /= np.linalg.norm(side)
        px = 2.0 / H

        def camera_at(k):
            sway = 2.0 * px * np.sin(0.7 * k)
            pos = [float(c + 0.01 * k * s) for c, s in zip(camera.position, side)]
            return E.Camera(pos, [float(v) for v in d0 + sway * side], camera.up)

        prev_view = E.View(camera, size, settings)
        guide_rt.first_hits_into(camera, guides[0].data_ptr())

    def step_moving():
        nonlocal frame, prev_view
        dst = targets[frame % len(targets)].data_ptr()
        cam = camera_at(frame)
        view = E.View(cam, size, settings)
        prev_hits, cur_hits = guides[(frame - 1) % len(guides)], guides[frame % len(guides)]
        if variant == "j":
            # the buffer's last reader was this context's upsample of two frames back: the writer follows it
            high_hits = high_guides[frame % 2]
            high_ctx.order_after(ctx)
            high_rt.first_hits_async(cam, high_hits.data_ptr())
        if variant == "k":
            off = E.history_phase(low_size, SIZE, frame)
            low_rt.shift_rays(*off)
            low_rt.compute(cam, frame)
            guide_rt.first_hits_async(cam, cur_hits.data_ptr())
            ctx.reproject_moments(prev_view, prev_hits.data_ptr(), view, cur_hits.data_ptr())
            ctx.accumulate_history_from(low_ctx, off, MAX_HISTORY, moments=True)
            tickets.append(ctx.denoise_variance_present(dst, nbytes, W, H, guide_ptr=cur_hits.data_ptr()))
            if len(tickets) > LAG:
                ctx.present_wait(tickets[-1 - LAG])
            prev_view = view
            frame += 1
            return
        if variant == "m":
            rt = raytraces[0]
            prev_state, state = states[(frame - 1) % 8], states[frame % 8]
            t_set = time.perf_counter()
            ctx.set_scene(rt.rays, rt.spheres, state[0], state[1])
            set_scene_s[0] += time.perf_counter() - t_set
            guide_rt.first_hits_async(cam, cur_hits.data_ptr())
            rt.compute(cam, frame)
            table = [E.motion_between(prev_state[2], state[2])] + [still] * (len(state[1]) - 1)
            ctx.reproject_motion(prev_view, prev_hits.data_ptr(), view, cur_hits.data_ptr(), meshes=table, moments=True)
            diffuses[0].next_frame_history(rt.image(), MAX_HISTORY, moments=True)
            tickets.append(ctx.denoise_variance_present(dst, nbytes, W, H, guide_ptr=cur_hits.data_ptr()))
            if len(tickets) > LAG:
                ctx.present_wait(tickets[-1 - LAG])
            prev_view = view
            frame += 1
            return
        if variant in ("h", "i", "j"):
            guide_rt.first_hits_async(cam, cur_hits.data_ptr())
        else:
            guide_rt.first_hits_into(cam, cur_hits.data_ptr())  # blocking
        raytraces[0].compute(cam, frame)
        if variant in ("i", "j"):
            ctx.reproject_moments(prev_view, prev_hits.data_ptr(), view, cur_hits.data_ptr())
            diffuses[0].next_frame_history(raytraces[0].image(), MAX_HISTORY, moments=True)
            if variant == "j":
                ctx.order_after(high_ctx)
                tickets.append(ctx.upsample_present(dst, nbytes, W, H, cur_hits.data_ptr(), high_hits.data_ptr(),
                                                    variance=vinfo))
            else:
                tickets.append(ctx.denoise_variance_present(dst, nbytes, W, H, guide_ptr=cur_hits.data_ptr()))
        else:
            ctx.reproject(prev_view, prev_hits.data_ptr(), view, cur_hits.data_ptr())
            diffuses[0].next_frame_history(raytraces[0].image(), MAX_HISTORY)
            tickets.append(ctx.denoise_present(dst, nbytes, W, H, guide_ptr=cur_hits.data_ptr()))
        if len(tickets) > LAG:
            ctx.present_wait(tickets[-1 - LAG])
        prev_view = view
        frame += 1

    def step():
        nonlocal frame
        if moving:
            return step_moving()
        dst = targets[frame % len(targets)].data_ptr()
        for raytrace in raytraces:
            raytrace.compute(camera, frame)
        if variant == "d":  # (on a group's root: accumulates on every part, then the gathered present)
            tickets.append(ctx.accumulate_present(frame, dst, nbytes, W, H))
        else:
            for raytrace, diffuse in zip(raytraces, diffuses):
                diffuse.next_frame(frame, raytrace.image())
            if variant == "b":
                ctx.read_into(_lib.IMG_ACCUM, _lib.FMT_RGBA8, dst, nbytes)
            elif variant == "c":
                tickets.append(ctx.present(_lib.IMG_ACCUM, dst, nbytes, W, H))
            elif variant == "e":
                tickets.append(ctx.denoise_present(dst, nbytes, W, H, guide_ptr=guide.data_ptr()))
        if len(tickets) > LAG:  # the frame of three back is on screen before its target is reused
            ctx.present_wait(tickets[-1 - LAG])
        frame += 1

    for _ in range(WARMUP):
        step()
    for c in ctxs:
        c.synchronize()
    if variant == "m":
        set_scene_s[0] = 0.0
    t0 = time.perf_counter()
    for _ in range(FRAMES):
        step()
    if variant == "j":
        high_ctx.synchronize()
    if variant == "k":
        low_ctx.synchronize()
    for c in reversed(ctxs):  # (the root last: its tickets follow every part's copy)
        c.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / FRAMES
    st = ctx.stats()
    if variant == "k":  # (the traces ran on the half-size context)
        size, last_kernel = low_size, low_ctx.stats().last_kernel
    else:
        last_kernel = st.last_kernel
    assert all(c.stats().accumulates == st.accumulates for c in ctxs)
    out = {"variant": variant, "parts": parts, "ms_per_frame": round(ms, 4), "frames": FRAMES, "warmup": WARMUP, "scene": SCENE,
           "width": W, "height": H, "render_width": size[0], "render_height": size[1], "spp": SPP, "bounces": BOUNCES, "kernel": _lib.KERNEL_NAMES[last_kernel],
           "accumulates": st.accumulates, "tickets": len(tickets), "build_id": _lib.build_id()}
    if variant == "m":
        out["set_scene_ms_per_frame"] = round(set_scene_s[0] * 1e3 / FRAMES, 4)
    if variant == "g":
        guide_ctx.close()
    if variant == "j":
        high_ctx.close()
    if variant == "k":
        low_ctx.close()
    for c in ctxs:
        c.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", choices=VARIANTS + ("e", "f", "g", "h", "i", "j", "k", "m"), help="run one variant in this process (what the driver starts)")
    ap.add_argument("--parts", type=int, default=1, help="contexts of 8-row tiles on device 0, joined as one group")
    ap.add_argument("--out", default=None, help="default profiles/present_loop.jsonl (present_loop_group.jsonl "
                                                "with --parts above 1, appended to)")
    ap.add_argument("--denoise", action="store_true",
                    help="variants c and e (hrt_denoise_present in place of hrt_present) only, taking turns")
    ap.add_argument("--moving", action="store_true",
                    help="variants e, f (the temporal pipeline with a moving camera), g (f with the first hits "
                         "taken on a second context) and h (f with hrt_first_hits, nothing blocking) only, taking turns")
    ap.add_argument("--variance", action="store_true",
                    help="variants h and i (h with the moments calls and the variance-guided filter) only, taking turns")
    ap.add_argument("--upsample", action="store_true",
                    help="variants i and j (i rendered at half size and shown through hrt_upsample_present) only, taking turns")
    ap.add_argument("--resolve", action="store_true",
                    help="variants i, j and k (the trace at half size on a shifted grid, the history at full size through "
                         "hrt_accumulate_history_from) only, taking turns")
    ap.add_argument("--objects", action="store_true",
                    help="variants i and m (i with one object moved every frame: hrt_set_scene and "
                         "hrt_reproject_motion_moments) only, taking turns")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None,
                    help="another build of libhip_raytrace.so (same ABI): each repeat also runs variant b on it "
                         "(HRT_LIB), alternating with this build's variants, recorded as b_baseline")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child process")
    a = ap.parse_args()
    if a.parts < 1:
        ap.error("--parts must be at least 1")
    if a.variant:
        print(json.dumps(child(a.variant, a.parts)), flush=True)
        return 0
    if (a.denoise or a.moving or a.variance or a.upsample or a.resolve or a.objects) and a.parts > 1:
        ap.error("--denoise, --moving and --variance run on a single context (a partitioned context cannot denoise or keep "
                 "history)")
    if a.out is None:
        name = "present_loop_motion.jsonl" if a.objects else "present_loop_resolve.jsonl" if a.resolve else "present_loop_upsample.jsonl" if a.upsample else "present_loop_variance.jsonl" if a.variance else "present_loop_history.jsonl" if a.moving else "present_loop_denoise.jsonl" if a.denoise else "present_loop_group.jsonl" if a.parts > 1 else "present_loop.jsonl"
        a.out = os.path.join(ROOT, "profiles", name)
    variants = OBJECTS_VARIANTS if a.objects else RESOLVE_VARIANTS if a.resolve else UPSAMPLE_VARIANTS if a.upsample else VARIANCE_VARIANTS if a.variance else MOVING_VARIANTS if a.moving else DENOISE_VARIANTS if a.denoise else VARIANTS
    order = ([("b_baseline", "b", a.baseline_lib)] if a.baseline_lib else []) + [(v, v, None) for v in variants]
    runs = {name: [] for name, _, _ in order}
    lines = []
    for rep in range(a.repeats):
        for name, v, lib in order:
            env = dict(os.environ, HRT_LIB=os.path.abspath(lib)) if lib else None
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v, "--parts", str(a.parts)],
                                   capture_output=True, text=True, timeout=a.timeout, env=env)
            except subprocess.TimeoutExpired:
                print(f"variant {v} repeat {rep}: no result within {a.timeout} s; stopping", file=sys.stderr)
                return 1
            rec = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
            if p.returncode != 0 or rec is None:
                print(f"variant {v} repeat {rep} failed ({p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
                return 1
            d = dict(json.loads(rec), repeat=rep, run=name)
            runs[name].append(d["ms_per_frame"])
            lines.append(json.dumps(d))
            print(lines[-1], flush=True)
    med = {v: statistics.median(runs[v]) for v in runs}
    summary = {"parts": a.parts,
               "summary": {v: {"median_ms": round(med[v], 4), "min_ms": min(runs[v]), "max_ms": max(runs[v]),
                               "spread_ms": round(max(runs[v]) - min(runs[v]), 4)} for v in runs}}
    if a.objects:
        sets = [json.loads(ln)["set_scene_ms_per_frame"] for ln in lines if json.loads(ln).get("run") == "m"]
        summary.update(m_over_i=round(med["m"] / med["i"], 4), m_minus_i_ms=round(med["m"] - med["i"], 4),
                       set_scene_median_ms=round(statistics.median(sets), 4),
                       set_scene_share_of_m=round(statistics.median(sets) / med["m"], 4),
                       ranges_apart=max(runs["m"]) < min(runs["i"]) or max(runs["i"]) < min(runs["m"]))
    elif a.resolve:
        lo_ms, hi_ms = sorted((med["j"], med["i"]))
        summary.update(k_over_i=round(med["k"] / med["i"], 4), k_over_j=round(med["k"] / med["j"], 4),
                       k_minus_j_ms=round(med["k"] - med["j"], 4), k_minus_i_ms=round(med["k"] - med["i"], 4),
                       k_between_j_and_i=lo_ms <= med["k"] <= hi_ms,
                       k_i_ranges_apart=max(runs["k"]) < min(runs["i"]) or max(runs["i"]) < min(runs["k"]),
                       k_j_ranges_apart=max(runs["k"]) < min(runs["j"]) or max(runs["j"]) < min(runs["k"]))
    elif a.upsample:
        summary.update(j_over_i=round(med["j"] / med["i"], 4), j_minus_i_ms=round(med["j"] - med["i"], 4),
                       ranges_apart=max(runs["j"]) < min(runs["i"]) or max(runs["i"]) < min(runs["j"]))
    elif a.variance:
        summary.update(i_over_h=round(med["i"] / med["h"], 4), i_minus_h_ms=round(med["i"] - med["h"], 4))
    elif a.moving:
        summary.update(f_over_e=round(med["f"] / med["e"], 4), f_minus_e_ms=round(med["f"] - med["e"], 4),
                       g_over_e=round(med["g"] / med["e"], 4), g_minus_e_ms=round(med["g"] - med["e"], 4),
                       f_minus_g_ms=round(med["f"] - med["g"], 4),
                       h_over_e=round(med["h"] / med["e"], 4), h_minus_e_ms=round(med["h"] - med["e"], 4),
                       f_minus_h_ms=round(med["f"] - med["h"], 4), g_minus_h_ms=round(med["g"] - med["h"], 4))
    elif a.denoise:
        summary.update(e_over_c=round(med["e"] / med["c"], 4), e_minus_c_ms=round(med["e"] - med["c"], 4))
    else:
        summary.update(c_over_b=round(med["c"] / med["b"], 4), d_over_c=round(med["d"] / med["c"], 4),
                       d_minus_c_ms=round(med["d"] - med["c"], 4))
    if a.baseline_lib:
        summary["b_over_b_baseline"] = round(med["b"] / med["b_baseline"], 4)
    lines.append(json.dumps(summary))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.parts > 1 else "w") as f:  # (the group file holds one run per --parts)
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
