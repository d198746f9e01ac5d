#!/usr/bin/env python3
"""Write tests/golden/glsl_ref.json: SHA-256 digests of the frames the reference's own shader text computes
(oracle/glsl_ref/, built by `make -C oracle glsl_ref` where a reference checkout exists) for the configurations of
tests/glsl_ref_cases.py GOLDEN_CONFIGS -- texels, stored floats, triangle-test count.  tests/test_glsl_ref.py compares
the ORACLE with these in every checkout.  Only digests and counts are stored: no shader text, nothing compiled."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import glsl_ref_cases as G  # noqa: E402
import pyoracle  # noqa: E402


def main() -> int:
    if pyoracle.load_glsl_ref() is None:
        print("no reference checkout and no built oracle/_ref/libglslref.so", file=sys.stderr)
        return 1
    frames = {}
    for cfg in G.GOLDEN_CONFIGS:
        case = G.case_of(cfg)
        g8, g32, tests = pyoracle.glsl_trace(case.push(), case.rays, case.spheres, case.tris, case.meshes)
        frames[G.config_id(cfg)] = G.digests(g8, g32, tests)
    with open(G.GOLDEN, "w") as f:
        json.dump({"source": "assets/raytracing.glsl compiled through oracle/glsl_ref (clang++, S1-S7)", "frames": frames},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(frames)} frames to {G.GOLDEN}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
