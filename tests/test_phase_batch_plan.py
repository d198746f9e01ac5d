"""The launch plan's primary threshold (epq_raytracer_amd/csrc/hrt_launch_plan.h), CPU only: the
new KernelTraits / LaunchPlan column resolves per kernel row and by the scene's bvh_node_r exactly as sec_batch
does, and a request of 0 takes the row's value.  tests/cpp/phase_batch_plan_test.cpp, compiled as plain C++
against the header, prints them; the values expected here are restated by hand."""
import json
import os
import re
import subprocess

from helpers import ROOT, _lib

SRC = os.path.join(ROOT, "tests", "cpp", "phase_batch_plan_test.cpp")
INC = [os.path.join(ROOT, "epq_raytracer_amd", "csrc"), os.path.join(ROOT, "include")]
WQ, WQ_L2 = 9, 10
# auto thresholds (whole-scene R, per-node R): the bounce thresholds as they were; primary 48 for BUNDLE_WQ, else 1
SEC = {k: (48, 48) for k in range(9)} | {WQ: (28, 36), WQ_L2: (28, 36)}
PRIM = {k: (1, 1) for k in range(9)} | {WQ: (48, 48), WQ_L2: (1, 1)}
REQUESTS = (0, 1, 28, 64)


def test_primary_threshold_resolves_per_row(tmp_path):
    exe = str(tmp_path / "phase_batch_plan_test")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                        *[f"-I{d}" for d in INC], SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, *map(str, REQUESTS)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(line) for line in r.stdout.splitlines()]
    assert [(d["kernel"], d["node_r"]) for d in recs] == [(k, n) for k in range(11) for n in (0, 1)]
    for d in recs:
        k, n = d["kernel"], d["node_r"]
        assert d["row"] == [*SEC[k], *PRIM[k]], d
        assert d["plan"] == [SEC[k][n], PRIM[k][n]], d  # the column of the scene's bvh_node_r, as for sec_batch
        assert 1 <= d["plan"][1] <= 64, d
        # 0 takes the row's value; any other request is the launch's
        assert d["resolved"] == [[q or SEC[k][n], q or PRIM[k][n]] for q in REQUESTS], d
    assert {d["kernel"] for d in recs if d["pairs"]} == {WQ, WQ_L2}


def test_option_and_diagnostics_mirrors():
    hdr = open(os.path.join(ROOT, "include", "hip_raytrace.h")).read()
    assert re.search(r"\bHRT_OPT_PRIMARY_BATCH = 22\b", hdr) and _lib.OPT_PRIMARY_BATCH == 22
    assert re.search(r"\bHRT_DIAG_PRIMARY_DEFERRED = 30\b", hdr) and re.search(r"\bHRT_DIAG_BATCH_ONLY_ITERS = 31\b", hdr)
    assert re.search(r"\bHRT_NUM_DIAG = 32\b", hdr) and len(_lib.DIAG_NAMES) == 32
    assert _lib.DIAG_NAMES[30:] == ("primary_deferred", "batch_only_iters")
    assert _lib.ABI_VERSION == 6  # additive: no bump
