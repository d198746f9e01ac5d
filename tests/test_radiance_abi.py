"""Radiance queries on the CPU (hrt_radiance): the layouts of hrt_radiance_query and
hrt_radiance_stats (a compiled C probe against the numpy / ctypes mirrors), the export from both libraries, the
NULL-handle rejection, and the Rust declarations INTEGRATION.md and the patch carry against the header."""
import ctypes
import os
import subprocess

import numpy as np

import test_rust_binding as RB
from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_FIELDS = ("origin", "seed", "centre", "reserved")
STATS_FIELDS = ("method_ran", "reserved", "scan_segments", "segments", "tri_tests")


def test_struct_layouts(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %zu %u\\n", sizeof(hrt_radiance_query), sizeof(hrt_radiance_stats), HRT_ABI_VERSION);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_radiance_query, {f}));\n' for f in QUERY_FIELDS)
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_radiance_stats, {f}));\n' for f in STATS_FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [32, 32, 6]  # additive: the ABI version stays 6
    assert _lib.ABI_VERSION == 6
    dt = _lib.RADIANCE_QUERY_DTYPE
    assert dt.names == QUERY_FIELDS and dt.itemsize == 32
    assert [dt.fields[f][1] for f in QUERY_FIELDS] == out[3:7] == [0, 12, 16, 28]
    cls = _lib.RadianceStats
    assert [n for n, _ in cls._fields_] == list(STATS_FIELDS)
    assert [getattr(cls, f).offset for f in STATS_FIELDS] == out[7:] == [0, 4, 8, 16, 24]
    assert ctypes.sizeof(cls) == 32
    header = open(os.path.join(ROOT, "include", "hip_raytrace.h")).read()
    assert "HRT_STATIC_ASSERT(sizeof(hrt_radiance_query) == 32" in header
    assert "HRT_STATIC_ASSERT(sizeof(hrt_radiance_stats) == 32" in header
    assert "#define HRT_ABI_VERSION 6u" in header and "hrt_radiance_query, hrt_radiance_stats" in header


def test_symbol_exported_from_both_libraries():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
        assert "hrt_radiance" in exported, path
    assert "hrt_radiance" in _lib.EXPORTED_SYMBOLS
    for lib in (_lib.load(), _lib.load(debug=True)):
        assert lib.hrt_radiance.argtypes and len(lib.hrt_radiance.argtypes) == 7


def test_null_handle_is_rejected():
    lib = _lib.load()
    queries = np.zeros(40, _lib.RADIANCE_QUERY_DTYPE)
    rgba = np.full((40, 4), -7.0, np.float32)
    st = _lib.RadianceStats(9, 9, 9, 9, 9)
    pc = _lib.PushConstants()
    assert lib.hrt_radiance(None, ctypes.byref(pc), _lib.ptr(queries), 40, _lib.QUERY_SCAN, _lib.ptr(rgba),
                            ctypes.byref(st)) == 1
    assert (rgba == -7.0).all() and (st.method_ran, st.scan_segments, st.segments, st.tri_tests) == (9, 9, 9, 9)


def test_integration_declares_the_structs_and_the_function():
    """INTEGRATION.md's Rust excerpt and the binding of the patch declare both structs and hrt_radiance as the
    header does (test_rust_binding's checker: field names, types, sizes, offsets, parameters)."""
    doc = open(RB.DOC).read()
    for src, text, rust in (("INTEGRATION.md", RB._rust_source(doc), False), ("src/hrt_ffi.rs", RB.ffi_text(), True)):
        plain = text if not rust else RB._strip_rust_comments(text)
        structs, fns = RB.rust_structs(plain), RB.rust_fns(plain)
        assert [f for f, _ in structs["hrt_radiance_query"]] == list(QUERY_FIELDS), src
        assert RB.rust_layout(structs["hrt_radiance_query"], structs) == (32, 4, [0, 12, 16, 28]), src
        assert [f for f, _ in structs["hrt_radiance_stats"]] == list(STATS_FIELDS), src
        assert RB.rust_layout(structs["hrt_radiance_stats"], structs) == (32, 8, [0, 4, 8, 16, 24]), src
        params, ret = fns["hrt_radiance"]
        assert [p for p, _ in params] == ["ctx", "pc", "queries", "n", "method", "rgba", "stats"] and ret == "i32", src
        assert dict(params)["rgba"] == "*mut f32" and dict(params)["stats"] == "*mut hrt_radiance_stats", src
        assert dict(params)["queries"] == "*const hrt_radiance_query", src
    assert not RB.check_binding(doc, complete=False)
    assert not RB.check_binding(RB.ffi_text(), rust=True)
    # ... and the checker sees a drifted declaration
    drift = doc.replace("method: u32, rgba: *mut f32, stats: *mut hrt_radiance_stats",
                        "method: u32, rgba: *mut f64, stats: *mut hrt_radiance_stats")
    assert drift != doc and any("hrt_radiance" in e for e in RB.check_binding(drift, complete=False))
