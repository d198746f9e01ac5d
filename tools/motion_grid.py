#!/usr/bin/env python3
"""What following a moving object buys on the CPU: tests/motion_ref.py on the CPU oracle's frames of
spheres and box at 64 x 64, 1 spp, 8 bounces, RGBA32F, the camera at rest.  One object moves between two states of the
scene: 16 frames of the old state are folded into a history, the history is carried to the new state, then 1, 2 and 4
frames of the new state are folded in (max_history 32).  Three ways to carry it:
  (a) hrt_reproject_motion with hrt_host_motion_between of the object's two poses (BILINEAR, default thresholds);
  (b) hrt_reproject on the same inputs: the motion ignored;
  (c) a restart: no history at all.
The error is the mean squared error of the rgb against the mean of 256 other frames traced in the new state, taken
over the pixels the mover covers now.  Moves: spheres -- the Lambertian ground (index 0) by 0.45 along x (2 to 3
pixels), the green mirror sphere (index 3) by 0.45 along x and by 1.7 upwards (about 10); box -- the mirror sphere (index 0) by 0.12 and by 0.47 along z, and the floor (mesh 0) turned
by 0.12 rad about its centre in its own plane.  Prints one JSON line per move with the share of the mover's pixels
that keep history under (a) and (b).
Usage: python tools/motion_grid.py"""
import copy
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
import motion_ref as M  # noqa: E402
from helpers import SceneCase  # noqa: E402

F32 = np.float32
SIZE = (64, 64)
OLD_FRAMES, NEW_FRAMES, TARGET_FRAMES = 16, (1, 2, 4), 256
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
MOVES = (("spheres", "sphere 0 (the ground) by 0.45 along x", ("sphere", 0, (0.45, 0.0, 0.0))),
         ("spheres", "sphere 3 by 0.45 along x", ("sphere", 3, (0.45, 0.0, 0.0))),
         ("spheres", "sphere 3 by 1.7 upwards", ("sphere", 3, (0.0, 1.7, 0.0))),
         ("box", "sphere 0 by 0.12 along z", ("sphere", 0, (0.0, 0.0, 0.12))),
         ("box", "sphere 0 by 0.47 along z", ("sphere", 0, (0.0, 0.0, 0.47))),
         ("box", "floor turned by 0.12 rad", ("mesh", 0, 0.12)))


def moved_case(name, move):
    """(the case of the new state, the mover's pose in it); move None: the old state, the identity."""
    camera, settings = E.preset(name)
    pose = np.array(IDENTITY, F32)
    if move is not None:
        kind, index, how = move
        if kind == "sphere":
            s = settings.sphere_data[index]
            t = np.array(how, F32)
            settings.sphere_data[index] = E.Sphere([float(F32(F32(c) + d)) for c, d in zip(s.centre, t)], s.radius, s.material)
            pose[9:] = t
        else:
            m = copy.deepcopy(settings.mesh_data[index])
            pos = np.asarray(m.mesh.positions, np.float64).reshape(-1, 3)
            centre = (pos.min(0) + pos.max(0)) / 2
            c, s = np.cos(how), np.sin(how)
            r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
            pose = np.concatenate([r.T.reshape(9), centre - r @ centre]).astype(F32)
            r32, t32 = pose[:9].reshape(3, 3).T.astype(np.float64), pose[9:].astype(np.float64)
            m.mesh.positions = (pos @ r32.T + t32).astype(F32).reshape(np.asarray(m.mesh.positions).shape)
            settings.mesh_data[index] = m
    return SceneCase(name, SIZE, num_samples=1, max_bounces=8, settings=settings, camera=camera), pose


def frames(case, first, n):
    return [case.oracle(rng_offset=first + k, want_f32=True)[1] for k in range(n)]


def fold(acc, cnt, new):
    return H.accumulate_history(acc, cnt, new, 32)


def grid_row(name, label, move):
    """One move: {"a": [mse after 1, 2, 4 frames], "b": ..., "c": ..., the kept shares}."""
    from test_history_ref import first_hits
    old_case, old_pose = moved_case(name, None)
    new_case, new_pose = moved_case(name, move)
    hp, hc = first_hits(old_case), first_hits(new_case)
    view = E.View(old_case.camera, SIZE, old_case.settings).record
    acc = np.zeros(SIZE[::-1] + (4,), F32)
    cnt = np.zeros(SIZE[::-1], np.uint32)
    for f in frames(old_case, 1, OLD_FRAMES):
        acc, cnt = fold(acc, cnt, f)
    tgt, tcnt = np.zeros_like(acc), np.zeros_like(cnt)
    for f in frames(new_case, 2000, TARGET_FRAMES):
        tgt, tcnt = H.accumulate_history(tgt, tcnt, f, 1 << 24)
    g, flags = M.motion_between(old_pose, new_pose)
    kind, index, _ = move
    spheres, meshes = M.static(len(new_case.spheres)), M.static(len(new_case.meshes))
    tab = spheres if kind == "sphere" else meshes
    tab["m"][index], tab["flags"][index] = g, flags
    key = M.surface_keys(hc)
    mover = key == ((0x80000000 | index) if kind == "sphere" else index + 1)
    states = {"a": M.reproject(acc, cnt, view, hp, view, hc, spheres, meshes, H.BILINEAR, *H.DEFAULTS),
              "b": H.reproject(acc, cnt, view, hp, view, hc, H.BILINEAR, *H.DEFAULTS),
              "c": (np.zeros_like(acc), np.zeros_like(cnt))}
    row = {"scene": name, "move": label, "mover_pixels": int(mover.sum()),
           "kept_a": round(float((states["a"][1][mover] > 0).mean()), 4),
           "kept_b": round(float((states["b"][1][mover] > 0).mean()), 4), "mse": {k: [] for k in states}}
    t3 = tgt[..., :3].astype(np.float64)
    for n, f in enumerate(frames(new_case, 1000, max(NEW_FRAMES)), 1):
        for k in states:
            states[k] = fold(*states[k], f)
            if n in NEW_FRAMES:
                err = ((states[k][0][..., :3].astype(np.float64) - t3) ** 2).sum(-1)[mover].mean() / 3
                row["mse"][k].append(round(float(err), 6))
    return row


def main() -> int:
    for name, label, move in MOVES:
        print(json.dumps(grid_row(name, label, move)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
