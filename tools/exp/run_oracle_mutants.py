#!/usr/bin/env python3
"""Build each tools/exp/oracle_mutant_*.patch as a wrong oracle and show which tests of tests/test_glsl_ref.py catch it.

    python tools/exp/run_oracle_mutants.py [name ...]

Each patch is applied to a COPY of oracle/rt_oracle.c in a temporary directory, compiled with oracle/Makefile's flags
and handed to the tests through the ORC_LIB switch of oracle/pyoracle.py.  Nothing shipped is touched or rebuilt.
CPU only.  Needs the reference checkout (the tests compare the oracle with the shader's own text); the digest test
catches frame-level mutants without it.  DESIGN.md 2 records the result."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CFLAGS = ("-O2 -std=c11 -fPIC -shared -ffp-contract=off -fno-fast-math -fno-math-errno -frounding-math "
          "-fexcess-precision=standard -fopenmp -mfma").split()


def main(argv) -> int:
    patches = sorted(glob.glob(os.path.join(ROOT, "tools", "exp", "oracle_mutant_*.patch")))
    if argv[1:]:
        patches = [p for p in patches if any(n in os.path.basename(p) for n in argv[1:])]
    missed = 0
    for patch in patches:
        name = os.path.basename(patch)[len("oracle_mutant_"):-len(".patch")]
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "oracle"))
            shutil.copy(os.path.join(ROOT, "oracle", "rt_oracle.c"), os.path.join(tmp, "oracle"))
            subprocess.run(["patch", "-s", "-p1", "-i", patch], cwd=tmp, check=True)
            lib = os.path.join(tmp, "liborc_mutant.so")
            subprocess.run(["gcc", *CFLAGS, "-o", lib, os.path.join(tmp, "oracle", "rt_oracle.c"), "-lm"], check=True)
            r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "not gpu", "-p", "no:cacheprovider",
                                os.path.join(ROOT, "tests", "test_glsl_ref.py")], cwd=ROOT,
                               env=dict(os.environ, ORC_LIB=lib), capture_output=True, text=True)
        failed = re.findall(r"^FAILED \S+::(\S+)", r.stdout, flags=re.M)
        groups = sorted({re.sub(r"\[.*", "", f) for f in failed})
        print(f"{name}: {len(failed)} failing tests: " + (", ".join(groups) if groups else "NOT CAUGHT"))
        missed += not failed
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
