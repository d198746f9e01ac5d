"""Object motion in the temporal history on the CPU: the layouts of hrt_motion and hrt_motion_tables (a compiled C
probe against the ctypes mirrors), the constants, the exports of both libraries, the motion forms of the reprojection
kernel in the code object, and the NULL-handle rejection.  The change is additive: like every addition since version
6, it leaves HRT_ABI_VERSION at 6, which the ABI tests of the earlier additions pin."""
import ctypes
import os
import re
import subprocess

import motion_ref as M
from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hrt_reproject_motion", "hrt_reproject_motion_moments", "hrt_host_motion_between"}


def test_struct_layouts_and_constants(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\n#include "hrt_host.h"\nint main(void) {\n'
                   '  printf("%zu %zu %u %u %u %u\\n", sizeof(hrt_motion), sizeof(hrt_motion_tables), HRT_MOTION_MOVING,\n'
                   '         HRT_MOTION_MAX_OBJECTS, HRT_MOTION_RING, HRT_ABI_VERSION);\n'
                   '  printf("%zu %zu %zu\\n", offsetof(hrt_motion, m), offsetof(hrt_motion, flags), offsetof(hrt_motion, reserved));\n'
                   '  printf("%zu %zu %zu %zu\\n", offsetof(hrt_motion_tables, spheres), offsetof(hrt_motion_tables, n_spheres),\n'
                   '         offsetof(hrt_motion_tables, meshes), offsetof(hrt_motion_tables, n_meshes));\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:6] == [64, 32, 1, 65536, 4, 6]  # additive: the ABI version stays 6
    assert out[6:9] == [0, 48, 52] and out[9:] == [0, 8, 16, 24]
    assert [getattr(_lib.Motion, f).offset for f in ("m", "flags", "reserved")] == out[6:9]
    assert [getattr(_lib.MotionTables, f).offset for f in ("spheres", "n_spheres", "meshes", "n_meshes")] == out[9:]
    assert (ctypes.sizeof(_lib.Motion), ctypes.sizeof(_lib.MotionTables)) == (64, 32)
    assert (_lib.MOTION_MOVING, _lib.MOTION_MAX_OBJECTS, _lib.MOTION_RING, _lib.ABI_VERSION) == (1, 65536, 4, 6)
    assert (M.MOVING, M.MAX_OBJECTS, M.MOTION.itemsize) == (1, 65536, 64)
    assert [M.MOTION.fields[f][1] for f in ("m", "flags", "reserved")] == out[6:9]
    assert _lib.load().hrt_abi_version() == 6


def test_symbols_exported_from_both_libraries():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
        assert NAMES <= exported, path
    assert NAMES <= set(_lib.EXPORTED_SYMBOLS)
    for lib in (_lib.load(), _lib.load(debug=True)):
        for n in NAMES:
            assert getattr(lib, n).argtypes, n


def test_motion_kernels_are_in_the_code_object():
    """The motion forms are reproject<T, Filter, Moments, true>, the plain ones reproject<T, Filter, Moments, false>:
    two texel types, two filters, with and without moments of each."""
    blob = open(_lib.LIB_PATH, "rb").read()
    found = set(re.findall(rb"_ZN3hrt9reprojectI(j|15HIP_vector_typeIfLj4EE)Lj([01])ELb([01])ELb([01])EEEv", blob))
    assert len(found) == 16 and len({f for f in found if f[3] == b"1"}) == 8, found


def test_null_handles_are_rejected():
    lib = _lib.load()
    info, view = _lib.ReprojectInfo(), _lib.View()
    lib.hrt_reproject_defaults(ctypes.byref(info))
    tables = _lib.MotionTables(None, 0, None, 0)
    for fn in (lib.hrt_reproject_motion, lib.hrt_reproject_motion_moments):
        assert fn(None, ctypes.byref(info), ctypes.byref(tables), ctypes.byref(view), None, ctypes.byref(view), None) == 1
