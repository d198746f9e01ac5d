#!/usr/bin/env python3
"""Rewrite the reference's two compute shaders into C++20 that compiles against glsl_shim.hpp.

    translate.py REFERENCE_DIR OUT_DIR

reads REFERENCE_DIR/assets/raytracing.glsl and image_combiner.glsl and writes OUT_DIR/raytracing_glsl.cpp and
OUT_DIR/image_combiner_glsl.cpp.  OUT_DIR is oracle/_ref/, which git ignores: nothing this writes is ever committed.

The rewrites are mechanical and local -- no statement of a shader is reordered, split or restated:
  * comments, `#version` and the `local_size` layout line are dropped;
  * `layout(.., rgba8) uniform image2D X;` becomes a plain `image2D X;`, a `buffer B { T[] x; };` block becomes a
    counted_buffer<T> x (a pointer whose operator[] counts), the push-constant block becomes a plain struct with a
    4-byte bool, and gl_GlobalInvocationID becomes a variable; all of them thread_local, one set per worker thread;
  * `inout T x` becomes `T& x`;
  * unsuffixed floating literals get an `f`, the `#define`s included (a GLSL literal is a float);
  * the `.xyz` swizzle becomes a call; `main` becomes `shader_main`;
  * the whole shader sits in a namespace of its own inside `glsl`, followed by the harness (`*_harness.inc`).
Anything else must already be C++.  Every identifier of the result has to be declared by the shader itself or belong
to the vocabulary below, and no qualifier, directive or swizzle other than the ones named above may remain: an
unknown construct stops the build here instead of reaching the compiler in some half-translated form.
"""
import os
import re
import sys

TYPES = {"void", "bool", "int", "uint", "float", "vec3", "vec4", "ivec2", "uvec3", "mat3", "mat4", "image2D",
         "bool32", "counted_buffer"}
KEYWORDS = {"if", "else", "for", "return", "continue", "break", "struct", "true", "false", "thread_local", "define",
            "undef"}
BUILTINS = {"dot", "cross", "normalize", "sqrt", "log", "sin", "cos", "min", "max", "mix", "reflect", "imageStore",
            "imageLoad", "gl_GlobalInvocationID", "x", "y", "z", "w", "xyz", "shader_main"}

FLOAT_LITERAL = re.compile(r"(?<![\w.])(\d+\.\d*(?:[eE][+-]?\d+)?|\.\d+(?:[eE][+-]?\d+)?|\d+[eE][+-]?\d+)(?![\w.])")
IMAGE = re.compile(r"layout\s*\(\s*set\s*=\s*\d+\s*,\s*binding\s*=\s*\d+\s*,\s*rgba8\s*\)\s*uniform\s+image2D\s+(\w+)\s*;")
BUFFER = re.compile(r"layout\s*\(\s*set\s*=\s*\d+\s*,\s*binding\s*=\s*\d+\s*\)\s*buffer\s+\w+\s*\{\s*(\w+)\s*\[\s*\]\s*(\w+)\s*;"
                    r"\s*\}\s*;")
PUSH = re.compile(r"layout\s*\(\s*push_constant\s*\)\s*uniform\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
LOCAL_SIZE = re.compile(r"layout\s*\(\s*local_size_x\s*=\s*\d+\s*,\s*local_size_y\s*=\s*\d+\s*,\s*local_size_z\s*=\s*\d+\s*\)"
                        r"\s*in\s*;")


class Unknown(Exception):
    pass


def strip_comments(src: str) -> str:
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def translate(src: str, namespace: str) -> str:
    src = strip_comments(src)
    src, n = re.subn(r"^\s*#version\s+460\s*$", "", src, count=1, flags=re.M)
    if n != 1:
        raise Unknown("expected one `#version 460`")
    src, n = LOCAL_SIZE.subn("", src)
    if n != 1:
        raise Unknown("expected one local_size layout")
    src = IMAGE.sub(r"thread_local image2D \1;", src)
    src = BUFFER.sub(r"thread_local counted_buffer<\1> \2;", src)

    def push(m):
        body = re.sub(r"\bbool\b", "bool32", m.group(2))
        return f"struct {m.group(1)} {{{body}}};\nthread_local {m.group(1)} {m.group(3)};"

    src, n = PUSH.subn(push, src)
    if n != 1:
        raise Unknown("expected one push-constant block")
    src = re.sub(r"\binout\s+(\w+)\s+(\w+)", r"\1& \2", src)
    src = FLOAT_LITERAL.sub(r"\1f", src)
    src = re.sub(r"\.xyz\b(?!\s*\()", ".xyz()", src)
    src = re.sub(r"\bvoid\s+main\s*\(\s*\)", "void shader_main()", src)

    check(src)
    defines = re.findall(r"^\s*#define\s+(\w+)", src, flags=re.M)
    head = ['#include "glsl_shim.hpp"'] + [f"#undef {d}" for d in defines]
    return "\n".join(head) + f"\nnamespace glsl {{\nnamespace {namespace} {{\nthread_local uvec3 gl_GlobalInvocationID;\n" \
        + src + f"\n}}  // namespace {namespace}\n}}  // namespace glsl\n"


def check(src: str) -> None:
    """Refuse whatever the rewrites above did not turn into the shim's C++."""
    for line in src.splitlines():
        s = line.strip()
        if s.startswith("#") and not re.fullmatch(r"#define\s+\w+\s+[0-9.eE+-]+f?", s):
            raise Unknown(f"directive: {s}")
    if re.search(r"(?<![\w.])\d+\.\d*(?![\dfeE])|(?<![\w.])\d+[eE][+-]?\d+(?![\df])", src):
        raise Unknown("a floating literal without a suffix is left")
    if re.search(r"\[\s*\]", src):
        raise Unknown("an unsized array is left")
    structs = set(re.findall(r"\bstruct\s+(\w+)", src))
    types = TYPES | structs
    words = re.findall(r"[A-Za-z_]\w*|\S", re.sub(r"\b\d[\w.+-]*", " ", src))
    declared = set(re.findall(r"#define\s+(\w+)", src))
    for a, b in zip(words, words[1:]):
        if a in types and re.fullmatch(r"[A-Za-z_]\w*", b):
            declared.add(b)
    for i, w in enumerate(words):  # `T& name`, `counted_buffer<T> name`
        if w in ("&", ">") and i + 1 < len(words) and i > 0 and words[i - 1] in types \
                and re.fullmatch(r"[A-Za-z_]\w*", words[i + 1]):
            declared.add(words[i + 1])
    for i, w in enumerate(words):
        if not re.fullmatch(r"[A-Za-z_]\w*", w):
            continue
        if i > 0 and words[i - 1] == "." and len(w) > 1 and set(w) <= set("xyzwrgbastpq") and w != "xyz":
            raise Unknown(f"swizzle .{w}")
        if w not in types and w not in KEYWORDS and w not in BUILTINS and w not in declared:
            raise Unknown(f"identifier `{w}` is neither declared by the shader nor part of the shim")


UNITS = (("raytracing.glsl", "raytracing", "rt_harness.inc"), ("image_combiner.glsl", "image_combiner", "combiner_harness.inc"))


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    ref, out = argv[1], argv[2]
    os.makedirs(out, exist_ok=True)
    for name, ns, harness in UNITS:
        path = os.path.join(ref, "assets", name)
        with open(path) as f:
            src = f.read()
        try:
            cpp = translate(src, ns)
        except Unknown as e:
            print(f"translate.py: {path}: {e}", file=sys.stderr)
            return 1
        with open(os.path.join(out, name.replace(".glsl", "_glsl.cpp")), "w") as f:
            f.write(f"// generated by oracle/glsl_ref/translate.py from the reference's assets/{name}; never committed\n")
            f.write(cpp + f'#include "{harness}"\n')
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
