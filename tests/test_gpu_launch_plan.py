"""The launch plan on the device (epq_raytracer_amd/csrc/hrt_launch_plan.h): every HRT_KERNEL_* request on three
scenes runs the kernel and workgroup size the commit before the plan existed ran -- hrt_stats.last_kernel and
last_block against tests/golden/launch_plan_parent.json -- and gives the oracle's bytes and counters, so that a
wrong LDS size or stack capacity shows as a mismatch and not only as the right kernel number.

The scenes: box (12 triangles: AUTO stays below the cull kernels), 70 one-triangle meshes (no hierarchy is
built: every hierarchy kernel falls back) and island with max_bounces = -1 (every request runs LITERAL).

The golden file is recorded by this module's own loop, run as a program with HRT_LIB naming the library of
the commit to record: `HRT_LIB=<its build>/libhip_raytrace.so python tests/test_gpu_launch_plan.py OUT COMMIT`."""
import json
import os
import sys

import numpy as np
import pytest

from helpers import E, ROOT, SceneCase, _lib, mismatch_report

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json")
KERNELS = range(_lib.KERNEL_BUNDLE_WQ_L2 + 1)  # 0 (AUTO) .. 10
SCENES = ["box", "meshes70", "island_no_bounce"]


def scene(name):
    """(case, push constants) of a scene."""
    if name == "box":
        case = SceneCase("box", (16, 16), 2, 4)
        return case, case.push()
    if name == "island_no_bounce":
        case = SceneCase("island", (48, 40), 2, 0)
        pc = case.push()
        pc.max_bounces = -1
        return case, pc
    rng = np.random.default_rng(5)  # tests/test_gpu_wq_l2.py test_fallback_without_a_hierarchy
    meshes = []
    for _ in range(70):
        c = rng.uniform(-4, 4, 3)
        v = (c + rng.uniform(-1, 1, (3, 3))).astype(np.float32)
        meshes.append(E.RayTracingMesh(E.Mesh(v, np.arange(3, dtype=np.uint32)),
                                       E.LambertianMaterial(list(rng.uniform(0.2, 0.9, 3)))))
    st = E.RayTracerSettings(num_samples=2, max_bounces=5, use_environment_lighting=True, mesh_data=meshes)
    case = SceneCase(settings=st, camera=E.Camera([0.0, 0.0, -12.0], [0.0, 0.0, 1.0]), size=(48, 40),
                     num_samples=2, max_bounces=5)
    return case, case.push()


def run(name):
    """One frame per requested kernel on one context: [(requested, last_kernel, last_block, image, segments,
    triangle tests)]."""
    case, pc = scene(name)
    ctx = case.context()
    out = []
    for k in KERNELS:
        ctx.set_option(_lib.OPT_KERNEL_VARIANT, k)
        ctx.reset_stats()
        ctx.trace(pc)
        st = ctx.stats()
        out.append((k, st.last_kernel, st.last_block, ctx.read(_lib.IMG_TRACE), st.segments, st.tri_tests))
    ctx.close()
    return out


@pytest.mark.parametrize("name", SCENES)
def test_every_request_runs_what_the_parent_ran(name):
    import pyoracle
    with open(GOLDEN) as f:
        golden = json.load(f)["plans"][name]
    case, pc = scene(name)
    ref, _, seg, tt = pyoracle.trace(pc, case.rays, case.spheres, case.tris, case.meshes)
    rows = run(name)
    assert [[k, ran, block] for k, ran, block, *_ in rows] == golden
    for k, ran, _, img, s, t in rows:
        assert np.array_equal(img, ref), f"{name} request {k} ran {ran}: " + mismatch_report(img, ref)
        assert (s, t) == (seg, tt), (name, k, ran)
    if name == "island_no_bounce":
        assert {ran for _, ran, *_ in rows} == {_lib.KERNEL_LITERAL}
    if name == "meshes70":  # no hierarchy kernel, whatever was asked for
        assert not {ran for _, ran, *_ in rows} & {_lib.KERNEL_BUNDLE_BVH, _lib.KERNEL_BUNDLE_BVH_LDS,
                                                   _lib.KERNEL_BUNDLE_WQ, _lib.KERNEL_BUNDLE_WQ_L2}


if __name__ == "__main__":
    plans = {name: [[k, ran, block] for k, ran, block, *_ in run(name)] for name in SCENES}
    with open(sys.argv[1], "w") as f:
        json.dump({"recorded_on_commit": sys.argv[2], "plans": plans}, f)
        f.write("\n")
