"""Temporal upsampling on the CPU: the layout of hrt_resolve_info (a compiled C probe against the ctypes mirror), the
constants, the defaults, the exports of both libraries, the kernels in the code object and the NULL-handle
rejection."""
import ctypes
import os
import subprocess

from epq_raytracer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("offset_x", "offset_y", "max_history", "flags", "reserved")
NAMES = {"hrt_resolve_defaults", "hrt_set_ray_grid", "hrt_history_phase", "hrt_accumulate_history_from"}


def test_struct_layout_and_constants(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hip_raytrace.h"\nint main(void) {\n'
                   '  printf("%zu %u %u %u\\n", sizeof(hrt_resolve_info), HRT_RESOLVE_FILL, HRT_RESOLVE_MOMENTS, '
                   'HRT_ABI_VERSION);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_resolve_info, {f}));\n' for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:4] == [32, _lib.RESOLVE_FILL, _lib.RESOLVE_MOMENTS, 6]  # additive: the ABI version stays 6
    assert (_lib.RESOLVE_FILL, _lib.RESOLVE_MOMENTS) == (1, 2)
    offsets = [0, 4, 8, 12, 16]
    assert out[4:] == offsets
    assert [n for n, _ in _lib.ResolveInfo._fields_] == list(FIELDS)
    assert [getattr(_lib.ResolveInfo, f).offset for f in FIELDS] == offsets
    assert ctypes.sizeof(_lib.ResolveInfo) == 32 and _lib.ABI_VERSION == 6
    assert _lib.load().hrt_abi_version() == 6


def test_the_header_compiles_as_cxx_with_its_static_asserts(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text('#include "hip_raytrace.h"\nstatic_assert(sizeof(hrt_resolve_info) == 32, "size");\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o",
                    str(tmp_path / "probe"), str(src)], check=True)


def test_defaults():
    for lib in (_lib.load(), _lib.load(debug=True)):
        info = _lib.ResolveInfo()
        ctypes.memset(ctypes.byref(info), 0xA5, 32)
        lib.hrt_resolve_defaults(ctypes.byref(info))
        assert (info.offset_x, info.offset_y, info.max_history, info.flags) == (0.0, 0.0, _lib.RESOLVE_MAX_HISTORY, _lib.RESOLVE_FILL)
        assert list(info.reserved) == [0, 0, 0, 0] and _lib.RESOLVE_MAX_HISTORY == 32
        lib.hrt_resolve_defaults(None)  # a NULL info is ignored


def test_symbols_exported_from_both_libraries():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
        assert NAMES <= exported, path
    assert NAMES <= set(_lib.EXPORTED_SYMBOLS)
    for lib in (_lib.load(), _lib.load(debug=True)):
        for n in NAMES:
            assert getattr(lib, n).argtypes, n


def test_kernels_are_in_the_code_object():
    blob = open(_lib.LIB_PATH, "rb").read()
    # Itanium mangling: resolve<T, Moments, Guided> with T = float4 (HIP_vector_type<float, 4>) or unsigned int
    for texel in (b"15HIP_vector_typeIfLj4EE", b"j"):
        for moments in (0, 1):
            for guided in (0, 1):
                k = b"_ZN3hrt7resolveI%sLb%dELb%dEEEv" % (texel, moments, guided)
                assert k in blob, k
    # the passes it shares its step and its ray grid with are still there
    assert b"fold_history" in blob and b"make_rays" in blob


def test_null_handles_are_rejected():
    lib = _lib.load()
    info = _lib.ResolveInfo()
    lib.hrt_resolve_defaults(ctypes.byref(info))
    v = _lib.f3((1.0, 0.0, 0.0))
    assert lib.hrt_set_ray_grid(None, v, v, v) == 1
    assert lib.hrt_accumulate_history_from(None, None, ctypes.byref(info), None, None) == 1
