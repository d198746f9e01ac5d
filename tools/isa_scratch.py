#!/usr/bin/env python3
"""Static counts and spill sites per kernel and per loop of a `make asm` listing:
    python3 tools/isa_scratch.py <hrt_kernels.s> [kernel name substring, default trace_bundle_wq]
Blocks are grouped by the innermost loop header the compiler's comments name, as in isa_loops.py, but
a block that is only fallen into (a "; %bb.N:" comment, no label) is taken for a block too -- isa_loops.py
counts it with the last label before it, often another loop's, so its totals differ by a few per cent.
Per loop: all / VALU / SALU / LDS instructions, the vector scratch accesses (loads, stores, and each
site's offset: `ld32` is a reload from scratch offset 32) and the v_readlane / v_writelane count (SGPR
spills to VGPR lanes and lane reads the source asks for are not told apart).  Nothing else is matched.
A loop's row holds only its own blocks, not those of the loops nested in it.  In trace_bundle_wq* the
fused sample loop is the depth-2 row of ~2,800, the pair step the depth-3 row of 550-680 with 26-34 LDS
instructions, the band round the depth-3 row with 12, the pool refill the depth-3 row of ~217 with none."""
import collections
import re
import sys

src = open(sys.argv[1]).read()
want = sys.argv[2] if len(sys.argv) > 2 else "trace_bundle_wq"


def kernel_names():
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)", src, re.M):
        if want in m.group(1):
            yield m.group(1)


def loops_of(name):
    start = src.index("\n" + name + ":") + 1
    end = src.index(".Lfunc_end", start)
    loops = collections.OrderedDict()
    cur = "entry"
    for l in src[start:end].splitlines()[1:]:
        s = l.strip()
        # a block starts at a label or, where it is only fallen into, at a "; %bb.N:" comment
        m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):\s*(;.*)?$", s)
        if m:
            c = m.group(2) or ""
            h = re.search(r"Header=BB(\d+_\d+) Depth=(\d+)", c)
            hl = re.search(r"Loop Header: Depth=(\d+)", c)
            if h:
                cur = "BB%s d%s" % (h.group(1), h.group(2))
            elif hl:
                cur = "%s d%s" % (m.group(1)[2:], hl.group(1))
            else:
                cur = "outside"
            continue
        if not s or s.startswith((".", ";", "//")):
            continue
        op = s.split()[0]
        d = loops.setdefault(cur, {"n": collections.Counter(), "sites": []})
        n = d["n"]
        n["all"] += 1
        if op.startswith("v_"):
            n["valu"] += 1
        elif op.startswith("s_"):
            n["salu"] += 1
        elif op.startswith("ds_"):
            n["lds"] += 1
        if op.startswith("scratch_"):
            off = re.search(r"offset:(\d+)", s)
            n["scratch_ld" if "load" in op else "scratch_st"] += 1
            d["sites"].append(("ld" if "load" in op else "st") + (off.group(1) if off else "0"))
        elif op.startswith(("v_readlane", "v_writelane")):
            n["lane"] += 1
    return loops


def resources(name):
    m = re.search(r"\.amdhsa_kernel\s+" + re.escape(name) + r"\b(.*?)\.end_amdhsa_kernel", src, re.S)
    out = {}
    for key in ("next_free_vgpr", "private_segment_fixed_size"):
        k = re.search(r"\.amdhsa_" + key + r"\s+(\d+)", m.group(1))
        out[key] = int(k.group(1)) if k else -1
    sp = re.search(r"\.name:\s+" + re.escape(name) + r"\n.*?\.vgpr_spill_count:\s*(\d+)", src, re.S)
    out["vgpr_spill"] = int(sp.group(1)) if sp else -1
    return out


for name in kernel_names():
    r = resources(name)
    print("%s  vgprs %d  scratch %d B/lane  vgpr spills %d" % (name, r["next_free_vgpr"],
                                                              r["private_segment_fixed_size"], r["vgpr_spill"]))
    print("  %-16s %6s %6s %6s %5s %4s %4s %5s  sites" % ("loop", "all", "valu", "salu", "lds", "sld", "sst", "lane"))
    for k, d in loops_of(name).items():
        n = d["n"]
        print("  %-16s %6d %6d %6d %5d %4d %4d %5d  %s" % (k, n["all"], n["valu"], n["salu"], n["lds"], n["scratch_ld"],
                                                            n["scratch_st"], n["lane"], " ".join(d["sites"])))
