"""The first-hit pass on the CPU: the layout of hrt_first_hits_stats (a compiled C probe against the ctypes
mirror), the enum and flag values, the exports of both libraries, the kernel's name in the code object and the
NULL-handle rejection."""
import ctypes
import os
import subprocess

import numpy as np

from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("method_ran", "reserved", "tiles", "tiles_listed", "tiles_empty", "tiles_fallback", "scan_rays", "tri_tests",
          "entries_tested")
NAMES = {"hrt_first_hits", "hrt_get_first_hits_stats"}


def test_struct_layout_and_constants(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %d %d %d %u %u\\n", sizeof(hrt_first_hits_stats), (int)HRT_FIRST_HITS_AUTO,\n'
                   '         (int)HRT_FIRST_HITS_TILES, (int)HRT_FIRST_HITS_QUERY, HRT_FIRST_HITS_COUNT, HRT_ABI_VERSION);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_first_hits_stats, {f}));\n' for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:6] == [48, 0, 1, 2, 1, 6]  # additive: the ABI version stays 6
    want = [0, 4, 8, 12, 16, 20, 24, 32, 40]
    assert out[6:] == want
    assert [n for n, _ in _lib.FirstHitsStats._fields_] == list(FIELDS)
    assert [getattr(_lib.FirstHitsStats, f).offset for f in FIELDS] == want
    assert ctypes.sizeof(_lib.FirstHitsStats) == 48
    assert (_lib.FIRST_HITS_AUTO, _lib.FIRST_HITS_TILES, _lib.FIRST_HITS_QUERY, _lib.FIRST_HITS_COUNT) == (0, 1, 2, 1)
    assert set(_lib.FIRST_HITS_NAMES) == {0, 1, 2} and _lib.ABI_VERSION == 6


def test_symbols_exported_from_both_libraries():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
        assert NAMES <= exported, path
    assert NAMES <= set(_lib.EXPORTED_SYMBOLS)
    for lib in (_lib.load(), _lib.load(debug=True)):
        for n in NAMES:
            assert getattr(lib, n).argtypes, n


def test_kernel_is_in_the_code_object():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert b"first_hits_tiles" in open(path, "rb").read(), path


def test_null_handles_are_rejected():
    for lib in (_lib.load(), _lib.load(debug=True)):
        pc = _lib.PushConstants()
        hits = np.full(64, 7, np.uint32)
        st = _lib.FirstHitsStats(9, 9, 9, 9, 9, 9, 9, 9, 9)
        for method in (_lib.FIRST_HITS_AUTO, _lib.FIRST_HITS_TILES, _lib.FIRST_HITS_QUERY):
            assert lib.hrt_first_hits(None, ctypes.byref(pc), method, 0, _lib.ptr(hits)) == 1
        assert lib.hrt_get_first_hits_stats(None, ctypes.byref(st)) == 1
        assert (hits == 7).all() and st.method_ran == 9 and st.entries_tested == 9  # nothing written
