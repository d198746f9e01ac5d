#!/usr/bin/env python3
"""Compares the compiled kernels of two builds: resource rows and instruction streams.

Input per side: the build directory `make asm` wrote its .s files into (epq_raytracer_amd/build) and the log of
that `make asm` run (its -Rpass-analysis=kernel-resource-usage remarks).  Output: a record in the form of
profiles/history_resources.txt -- for every kernel of the parent its resource row on both sides and whether its
instruction stream (labels, directives and comments stripped, branch targets without the function's index) is the parent's line for line, then the kernels
only the new build has.

  python tools/kernel_resources_diff.py PARENT_BUILD PARENT_LOG NEW_BUILD NEW_LOG > profiles/NAME.txt
"""
import glob
import os
import re
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]",
          "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def rows(log):
    """kernel -> its resource row, in the log's order"""
    out, name = {}, None
    for line in open(log):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return {k: " ".join(v.get(f, "?") for f in FIELDS) for k, v in out.items()}


def streams(build):
    """kernel -> its instructions (the lines between its label and its end marker that are instructions)"""
    out = {}
    for path in sorted(glob.glob(os.path.join(build, "*.s"))):
        name, body = None, []
        for line in open(path):
            s = line.split(";")[0].strip()
            m = re.match(r"^(_Z\w+):", s)
            if m and name is None:
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            if s.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            if not s or s.startswith(".") or s.endswith(":"):
                continue
            # a branch target .LBB<f>_<b> names block b of the unit's f-th function: f moves when a kernel is added
            # to the unit ahead of this one, the code does not
            body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s))
    return out


def main():
    pb, pl, nb, nl = sys.argv[1:5]
    prow, nrow, pstr, nstr = rows(pl), rows(nl), streams(pb), streams(nb)
    same = [k for k in prow if k in nrow and prow[k] == nrow[k] and pstr.get(k) == nstr.get(k)]
    print(f"## 1. every pre-existing kernel ({len(prow)} kernels; {len(same)} same, {len(prow) - len(same)} differing)")
    print("# " + ", ".join(FIELDS) + ": parent | this change;")
    print("# stream: the kernel's instructions with labels, directives and comments stripped, line for line against the parent's")
    for k in prow:
        if k not in nrow:
            print(f"gone   {k}\n      {prow[k]} | -")
            continue
        a, b = pstr.get(k, []), nstr.get(k, [])
        if a == b:
            what = f"stream identical ({len(a)} instructions)"
        else:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            what = f"stream DIFFERS ({len(a)} -> {len(b)} instructions, first at {first})"
        tag = "same  " if k in same else "DIFF  "
        print(f"{tag} {k}\n      {prow[k]} | {nrow[k]} | {what}")
    new = [k for k in nrow if k not in prow]
    print(f"\n## 2. the new kernels ({len(new)} kernels)")
    print("# " + ", ".join(FIELDS) + " | instructions")
    for k in new:
        print(f"new    {k}\n      {nrow[k]} | {len(nstr.get(k, []))} instructions")


if __name__ == "__main__":
    main()
