"""Occlusion queries on the CPU (hrt_occluded): the layout of hrt_occlusion_stats (a
compiled C probe against the ctypes mirror), the export from both libraries, the NULL-handle rejection, the Rust
declarations INTEGRATION.md quotes against the header, and plan_query -- which hrt_occluded calls unchanged --
against the rules of tests/test_launch_plan.py for the scene classes of tests/golden/launch_plan_parent.json."""
import ctypes
import json
import os
import subprocess

import numpy as np

import test_launch_plan as LP
import test_rust_binding as RB
from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("method_ran", "reserved", "scan_rays", "tri_tests", "occluded")


def test_struct_layout(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %u\\n", sizeof(hrt_occlusion_stats), HRT_ABI_VERSION);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_occlusion_stats, {f}));\n' for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:2] == [32, 6]  # additive: the ABI version stays 6
    assert _lib.ABI_VERSION == 6
    cls = _lib.OcclusionStats
    assert [n for n, _ in cls._fields_] == list(FIELDS)
    assert [getattr(cls, f).offset for f in FIELDS] == out[2:] == [0, 4, 8, 16, 24]
    assert ctypes.sizeof(cls) == 32
    # the header pins it too
    header = open(os.path.join(ROOT, "include", "hip_raytrace.h")).read()
    assert "HRT_STATIC_ASSERT(sizeof(hrt_occlusion_stats) == 32" in header
    assert "#define HRT_ABI_VERSION 6u" in header and "hrt_occlusion_stats, hrt_occluded" in header


def test_symbol_exported_from_both_libraries():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
        assert "hrt_occluded" in exported, path
    assert "hrt_occluded" in _lib.EXPORTED_SYMBOLS
    for lib in (_lib.load(), _lib.load(debug=True)):
        assert lib.hrt_occluded.argtypes and len(lib.hrt_occluded.argtypes) == 6


def test_null_handle_is_rejected():
    lib = _lib.load()
    rays = np.zeros(40, _lib.RAY_QUERY_DTYPE)
    bits = np.full(4, 0xCDCDCDCD, np.uint32)
    st = _lib.OcclusionStats(9, 9, 9, 9, 9)
    assert lib.hrt_occluded(None, _lib.ptr(rays), 40, _lib.QUERY_SCAN, _lib.ptr(bits), ctypes.byref(st)) == 1
    assert (bits == 0xCDCDCDCD).all() and (st.method_ran, st.scan_rays, st.tri_tests, st.occluded) == (9, 9, 9, 9)


def test_integration_declares_the_struct_and_the_function():
    """INTEGRATION.md's Rust excerpt and the binding of the patch declare hrt_occlusion_stats and hrt_occluded
    as the header does (test_rust_binding's checker: field names, types, sizes, offsets, parameters)."""
    doc = open(RB.DOC).read()
    for src, text, rust in (("INTEGRATION.md", RB._rust_source(doc), False), ("src/hrt_ffi.rs", RB.ffi_text(), True)):
        plain = text if not rust else RB._strip_rust_comments(text)
        structs, fns = RB.rust_structs(plain), RB.rust_fns(plain)
        assert [f for f, _ in structs["hrt_occlusion_stats"]] == list(FIELDS), src
        size, align, offs = RB.rust_layout(structs["hrt_occlusion_stats"], structs)
        assert (size, align, offs) == (32, 8, [0, 4, 8, 16, 24]), src
        params, ret = fns["hrt_occluded"]
        assert [p for p, _ in params] == ["ctx", "rays", "n", "method", "bits", "stats"] and ret == "i32", src
        assert dict(params)["bits"] == "*mut u32" and dict(params)["stats"] == "*mut hrt_occlusion_stats", src
    assert not RB.check_binding(doc, complete=False)
    assert not RB.check_binding(RB.ffi_text(), rust=True)
    # ... and the checker sees a drifted declaration
    drift = doc.replace("bits: *mut u32,\n                        stats: *mut hrt_occlusion_stats", "bits: *mut u64,\n"
                        "                        stats: *mut hrt_occlusion_stats")
    assert drift != doc and any("hrt_occluded" in e for e in RB.check_binding(drift, complete=False))


def test_plan_query_is_unchanged(tmp_path):
    """hrt_occluded resolves its method with plan_query as hrt_intersect does.  The planner's program over the
    grid of tests/test_launch_plan.py: every scene's four query plans are the rules' -- among them the classes
    the parent's recorded plans stand for: a hierarchy whose pair image fits (box), more than 64 meshes (every
    method runs the scan), and a scene without bounces (queries do not depend on the bounce count)."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json")))
    assert set(golden["plans"]) == {"box", "meshes70", "island_no_bounce"}
    exe, r = LP.build(tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    cases, _ = LP.trace_cases()
    recs = [json.loads(line) for line in LP.run(exe).splitlines()][:len(cases)]
    seen = set()
    for s, got in zip(cases, recs):
        want = LP.expected(s)["query"]
        assert got["query"] == want, s
        methods = [q[0] for q in got["query"]]
        if s["meshes"] > 64:
            assert methods == [LP.Q_SCAN] * 4, s
            seen.add("meshes70")
        elif methods == [LP.Q_BVH, LP.Q_SCAN, LP.Q_BVH, LP.Q_PAIRS]:
            assert 0 < got["query"][3][1] <= LP.MAX_LDS, s
            seen.add("box" if s["bounces"] > 0 else "island_no_bounce")
    assert seen == set(golden["plans"])
