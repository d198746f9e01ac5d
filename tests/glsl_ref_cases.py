"""Scenes, frame configurations and digests shared by tests/test_glsl_ref.py, tests/test_gpu_glsl_ref.py and
tests/golden/make_glsl_ref.py: the oracle and the kernels against the reference's own shader text
(oracle/glsl_ref/, DESIGN.md 2 "Parity status").  The constructed scenes are the GPU parity tests' own builders."""
from __future__ import annotations

import functools
import hashlib
import json
import os

import numpy as np

from helpers import E, ROOT, SceneCase

GOLDEN = os.path.join(ROOT, "tests", "golden", "glsl_ref.json")
PRESETS = ("box", "spheres", "island", "cave", "cube")
CONSTRUCTED = ("ties", "degenerate", "needle", "soup", "terrain_0", "terrain_0.01", "terrain_1.5", "invisible",
               "ten_meshes", "empty")
SCENES = PRESETS + CONSTRUCTED


def invisible_light_scene():
    """An invisible emitter between the camera and a Lambertian sphere, a second one above it, a mirror and a floor:
    camera rays meet the invisible sphere first (raytracing.glsl:323-326, the step along the ray), bounce rays meet
    it after a visible object (:321, the scalar offset).  Two more emitters carry a flag one ulp either side of 1.0:
    visible lights."""
    inv = E.InvisLightMaterial([1.0, 0.9, 0.8, 4.0])
    near = [np.nextafter(np.float32(1.0), np.float32(0.0)), np.nextafter(np.float32(1.0), np.float32(2.0))]
    spheres = [E.Sphere([0.0, 0.0, -3.0], 0.8, inv), E.Sphere([0.0, 2.5, 0.0], 1.0, inv),
               E.Sphere([0.0, 0.0, 0.0], 1.0, E.LambertianMaterial([0.8, 0.3, 0.3])),
               E.Sphere([2.2, 0.0, 0.5], 1.0, E.MetalMaterial([0.9, 0.9, 0.9], 1.0, 0.0)),
               E.Sphere([-2.2, 0.0, 0.5], 1.0, E.MetalMaterial([0.7, 0.8, 0.9], 0.5, 1.0)),
               E.Sphere([-1.5, 2.0, -1.0], 0.4, inv), E.Sphere([1.5, 2.0, -1.0], 0.4, inv)]
    floor = np.array([[-8, -1, -8], [8, -1, -8], [-8, -1, 8], [8, -1, 8]], np.float32)
    mesh = E.Mesh(floor, np.array([0, 2, 1, 1, 2, 3], np.uint32))
    st = E.RayTracerSettings(num_samples=3, max_bounces=8, use_environment_lighting=False, sphere_data=spheres,
                             mesh_data=[E.RayTracingMesh(mesh, E.LambertianMaterial([0.6, 0.6, 0.6]))])
    return st, E.Camera([0.0, 0.4, -7.0], [0.0, -0.05, 1.0]), near


def scene_case(name: str, size=(48, 36), spp=3, bounces=8, rng_offset=1, env=None, jitter=None) -> SceneCase:
    """A fresh SceneCase of the named scene; env / jitter override the scene's own."""
    if name in PRESETS:
        case = SceneCase(name, size, spp, bounces, rng_offset=rng_offset)
    else:
        near = None
        if name == "ties":
            import test_gpu_parity as P
            c = P._tie_soup()
            st, cam = c.settings, c.camera
        elif name == "degenerate":
            import test_gpu_intersect as TI
            c = TI.degenerate()
            st, cam = c.settings, c.camera
        elif name == "needle":
            import test_gpu_tile_cull as TC
            cam = E.Camera(*TC.NEEDLE_CAMERA)
            st = TC.needle_settings(cam, size)
        elif name == "soup":
            import test_gpu_parity as P
            st = E.RayTracerSettings(num_samples=spp, max_bounces=bounces, use_environment_lighting=True,
                                     mesh_data=[E.RayTracingMesh(P._soup(256), E.LambertianMaterial([0.5, 0.5, 0.5]))])
            cam = E.Camera([0.0, 0.0, -25.0], [0.0, 0.0, 1.0])
        elif name.startswith("terrain_"):
            import test_gpu_parity as P
            eye_y = float(name.split("_")[1])
            st = E.RayTracerSettings(
                num_samples=spp, max_bounces=bounces, use_environment_lighting=True,
                sphere_data=[E.Sphere([0.0, 0.5, 0.0], 0.5, E.LambertianMaterial([0.9, 0.3, 0.3]))],
                mesh_data=[E.RayTracingMesh(P._grid_terrain(), E.MetalMaterial([0.8, 0.8, 0.7], 0.9, 0.4)),
                           E.RayTracingMesh(P._grid_terrain(6, 2.0, 5, 9), E.LambertianMaterial([0.3, 0.6, 0.3]))])
            cam = E.Camera([-7.5, eye_y, -0.3], [1.0, -0.02 if eye_y > 0 else 0.0, 0.05])
        elif name == "invisible":
            st, cam, near = invisible_light_scene()
        elif name == "ten_meshes":
            import test_gpu_parity as P
            cam, st = P._island_split(3)
        elif name == "empty":
            st = E.RayTracerSettings(num_samples=spp, max_bounces=bounces, use_environment_lighting=True)
            cam = E.Camera([0, 0, 0], [1, 0.5, 0.2])
        else:
            raise KeyError(name)
        case = SceneCase(None, size, spp, bounces, rng_offset=rng_offset, settings=st, camera=cam)
        if near is not None:  # the last two spheres: flag 1.0 -/+ 1 ulp
            case.spheres = case.spheres.copy()
            case.spheres["material"]["settings"][-2:, 3] = near
    if env is not None:
        case.settings.use_environment_lighting = bool(env)
    if jitter is not None:
        case.jitter = float(np.float32(jitter))
    return case


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def bounce_like_rays(case, rng, n):
    """Origins on random triangles and spheres of the scene (where bounce rays start), random directions, and a
    share of camera rays."""
    o = np.zeros((n, 3), np.float32)
    pick = rng.random(n)
    if len(case.meshes):
        k = rng.integers(0, len(case.tris), n)
        uv = rng.dirichlet([1, 1, 1], n)
        t = case.tris[k]
        o = (t["a"][:, :3] + uv[:, :1] * t["edge_one"][:, :3] + uv[:, 1:2] * t["edge_two"][:, :3]).astype(np.float32)
    if len(case.spheres):
        s = case.spheres[rng.integers(0, len(case.spheres), n)]
        on = (s["centre"] + unit(rng.normal(size=(n, 3))) * s["radius"][:, None]).astype(np.float32)
        use = (pick < 0.4) | (len(case.meshes) == 0)
        o[use] = on[use]
    d = unit(rng.normal(size=(n, 3)))
    cam = pick > 0.8
    o[cam] = np.asarray(case.camera.position, np.float32)
    M = np.asarray(case.push().cam_alignment_mat, np.float64).reshape(4, 4).T[:3, :3]
    cen = case.rays["sample_centre"][rng.integers(0, len(case.rays), n), :3].astype(np.float64)
    d[cam] = unit(cen @ M.T)[cam]
    return o, d


# (spp, bounces, rng_offset, env (None: the scene's), jitter (None: the default))
BASE = (3, 8, 1, None, None)
VARIATIONS = ((1, 0, 0, None, None), (1, 1, 0xFFFFFFFF, False, None), (3, 1, 0, True, 0.0), (1, 8, 0xFFFFFFFF, None, 3.0e38),
              (3, 0, 1, False, 0.0))
SIZES = {"island": (40, 30), "cave": (40, 30), "ten_meshes": (40, 30), "box": (45, 33), "needle": (64, 40),
         "ties": (36, 28), "terrain_0": (48, 32), "terrain_0.01": (48, 32), "terrain_1.5": (48, 32)}


def frame_configs():
    """Every scene at its base parameters and at two of the variations (dealt round robin, so that each variation
    meets presets and constructed scenes), plus every variation on box and spheres."""
    out = []
    for k, name in enumerate(SCENES):
        size = SIZES.get(name, (48, 36))
        out.append((name, size) + BASE)
        picks = range(len(VARIATIONS)) if name in ("box", "spheres") else (k % len(VARIATIONS), (k + 2) % len(VARIATIONS))
        out += [(name, size) + VARIATIONS[v] for v in picks]
    return out


def config_id(cfg) -> str:
    name, size, spp, bounces, off, env, jitter = cfg
    return f"{name}-{size[0]}x{size[1]}-s{spp}-b{bounces}-o{off}-e{'scene' if env is None else int(env)}-j{jitter}"


def case_of(cfg) -> SceneCase:
    name, size, spp, bounces, off, env, jitter = cfg
    return scene_case(name, size, spp, bounces, off, env, jitter)


# the configurations whose shader digests are committed (tests/golden/glsl_ref.json)
GOLDEN_CONFIGS = (("box", (45, 33)) + BASE, ("spheres", (48, 36)) + BASE, ("island", (40, 30)) + BASE,
                  ("cave", (40, 30)) + BASE, ("cube", (48, 36)) + VARIATIONS[0], ("ties", (36, 28)) + BASE,
                  ("degenerate", (48, 36)) + VARIATIONS[1], ("invisible", (48, 36)) + BASE,
                  ("terrain_0", (48, 32)) + VARIATIONS[2], ("box", (45, 33)) + VARIATIONS[3],
                  ("ten_meshes", (40, 30)) + VARIATIONS[4])


def digests(img8: np.ndarray, img32: np.ndarray, tri_tests: int) -> dict:
    """SHA-256 of the texels and of the float words (every NaN as the one quiet NaN: S1 does not pin payloads)."""
    f = np.ascontiguousarray(img32, np.float32).copy()
    f[np.isnan(f)] = np.float32(np.nan)
    return {"sha256_rgba8": hashlib.sha256(np.ascontiguousarray(img8).tobytes()).hexdigest(),
            "sha256_rgba32f": hashlib.sha256(f.view(np.uint32).tobytes()).hexdigest(), "tri_tests": int(tri_tests)}


@functools.lru_cache(maxsize=None)
def golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)["frames"]
