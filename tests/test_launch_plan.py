"""Launch planning (epq_raytracer_amd/csrc/hrt_launch_plan.h: plan_trace, plan_query, the pair stacks and the
heavy-tile rule -- what hrt_kernels.hip's launch wrappers and hrt_api.cpp run), CPU only.  The test compiles
tests/cpp/launch_plan_test.cpp as plain C++ against the header, runs it over a grid of scenes and requests and
compares every field with the rules as DESIGN.md 23 words them, restated below by hand; once more with the
program built under ASan + UBSan."""
import ctypes
import itertools
import json
import os
import subprocess

import pytest

from helpers import ROOT, _lib

SRC = os.path.join(ROOT, "tests", "cpp", "launch_plan_test.cpp")
INC = [os.path.join(ROOT, "epq_raytracer_amd", "csrc"), os.path.join(ROOT, "include")]

AUTO, LITERAL, BRUTE, BRUTE_LDS, BUNDLE, CULL, BVH, CULL_LDS, BVH_LDS, WQ, WQ_L2 = range(11)
Q_AUTO, Q_SCAN, Q_BVH, Q_PAIRS = range(4)
MAX_LDS = 160 * 1024 - 64  # dynamic LDS a workgroup may ask for
COOP = 3 * 64 * 8          # BUNDLE_CULL_LDS's exchange slots
FIELDS = ("requested n_tris cam_cap meshes bounces nodes entries wq bfs sah bvh_nodes bvh_prims bvh_meshes "
          "wq_n width leaf node_r lds_opt ncap_req tcap_req").split()


# ---- the rules, restated ------------------------------------------------------------------------
def tri_cap(leaf):
    return 64 * (1 + 2 * leaf)


def stack_cap(n, width, leaf):
    """Node pairs per wave beside the whole image: what is left of the LDS, in 64s, at most 1024; 0: no fit."""
    if leaf > 4 or not 2 <= width <= 4:
        return 0
    if n * 48 + 16 * (512 + 4 * (tri_cap(leaf) + 128)) > MAX_LDS:
        return 0
    per_wave = (MAX_LDS - n * 48) // 16
    return min(1024, (per_wave - 512 - 4 * tri_cap(leaf)) // 4 // 64 * 64)


def capped(cap, request):
    return min(cap, max(128, request // 64 * 64)) if request else cap


def l2_plan(n, width, leaf, opt, nreq, treq):
    """(nodes in LDS, node pairs, triangle pairs, bytes); zeros: the kernel does not take the image."""
    if not 1 <= n < 65536 or not 1 <= leaf <= 4 or not 2 <= width <= 4:
        return (0, 0, 0, 0)
    t, nmax = capped(tri_cap(leaf), treq), capped(1024, nreq)

    def stacks(ncap):
        return 16 * (512 + 4 * (ncap + t))

    if stacks(128) > MAX_LDS:
        return (0, 0, 0, 0)
    if opt < 0:  # the stacks first, the nodes what is left
        ncap = nmax
        while stacks(ncap) > MAX_LDS:
            ncap -= 64
        keep = min(n, (MAX_LDS - stacks(ncap)) // 48)
    else:        # the nodes first (beside stacks of at least 128), the stacks what is left
        keep = min(opt, n, (MAX_LDS - stacks(128)) // 48)
        ncap = min(nmax, ((MAX_LDS - keep * 48) // 16 - 512 - 4 * t) // 4 // 64 * 64)
    return (keep, ncap, t, keep * 48 + stacks(ncap))


def scene_l2(s):
    if not (s["nodes"] and s["bfs"]):
        return (0, 0, 0, 0)
    return l2_plan(s["wq_n"], s["width"], s["leaf"], s["lds_opt"], s["ncap_req"], s["tcap_req"])


def cull_block(n_tris):
    lds = n_tris * 48 + COOP
    return 512 if lds <= MAX_LDS // 2 else 1024 if lds <= MAX_LDS else 0


def hierarchy_ok(s):
    return bool(s["nodes"]) and s["meshes"] <= 64


def wq_cap(s):
    return stack_cap(s["wq_n"], s["width"], s["leaf"]) if s["nodes"] and s["wq"] else 0


def fits(s, k):
    if k == BRUTE_LDS:
        return s["n_tris"] * 48 <= MAX_LDS
    if k == CULL_LDS:
        return cull_block(s["n_tris"]) != 0
    if k == BVH:
        return hierarchy_ok(s)
    if k == BVH_LDS:
        return hierarchy_ok(s) and bool(s["entries"]) and \
            s["n_tris"] * 48 + s["bvh_nodes"] * 64 + s["bvh_prims"] * 4 + s["bvh_meshes"] * 4 <= MAX_LDS
    if k == WQ:
        return hierarchy_ok(s) and wq_cap(s) != 0
    if k == WQ_L2:
        return hierarchy_ok(s) and scene_l2(s)[3] != 0
    return True


FALLBACK = {BRUTE_LDS: BRUTE, CULL_LDS: CULL, BVH: CULL, BVH_LDS: BVH, WQ: BVH_LDS, WQ_L2: BVH_LDS}
PERSISTENT, LISTS = {CULL_LDS, BVH_LDS, WQ, WQ_L2}, {BUNDLE, CULL, BVH, CULL_LDS, BVH_LDS, WQ, WQ_L2}
HIERARCHY = {BVH, BVH_LDS, WQ, WQ_L2}


def resolve(s, k):
    if k == AUTO:
        good = bool(s["nodes"]) and s["sah"] <= 100
        if s["cam_cap"] < 256:
            k = BUNDLE
        elif good and s["meshes"] <= 64 and wq_cap(s) >= 384:
            k = WQ
        elif s["cam_cap"] >= 4096 and good:
            k = BVH
        else:
            k = CULL_LDS if cull_block(s["n_tris"]) else CULL
    while not fits(s, k):
        k = FALLBACK[k]
    return LITERAL if s["bounces"] < 0 else k


def expected(s):
    k = resolve(s, s["requested"])
    e = dict(kernel=k, block=256, groups=0, lds=0, ncap=0, tcap=0, lnodes=0, split_k=1, sec_batch=48,
             fits=1, persistent=int(k in PERSISTENT), lists=int(k in LISTS), sky=int(k == WQ), pairs=int(k in (WQ, WQ_L2)))
    if k == BRUTE_LDS:
        e.update(block=1024, lds=s["n_tris"] * 48)
    elif k == CULL_LDS:
        e.update(block=cull_block(s["n_tris"]), lds=s["n_tris"] * 48 + COOP)
        e["groups"] = 2 if e["block"] == 512 else 1
    elif k == BVH_LDS:
        e.update(block=1024, groups=1,
                 lds=s["n_tris"] * 48 + s["bvh_nodes"] * 64 + s["bvh_prims"] * 4 + s["bvh_meshes"] * 4)
    elif k in (WQ, WQ_L2):
        e.update(block=1024, groups=1, split_k=8, sec_batch=36 if s["node_r"] else 28)
        if k == WQ:  # the bytes are sized for the whole stacks; the requests lower what the kernel is told
            n, t = wq_cap(s), tri_cap(s["leaf"])
            e.update(lds=s["wq_n"] * 48 + 16 * (512 + 4 * (n + t)), ncap=capped(n, s["ncap_req"]), tcap=capped(t, s["tcap_req"]))
        else:
            e["lnodes"], e["ncap"], e["tcap"], e["lds"] = scene_l2(s)
    query = []
    for m in range(4):
        m = Q_BVH if m == Q_AUTO else m
        if m == Q_PAIRS and not fits(s, WQ):
            m = Q_BVH
        if m == Q_BVH and not hierarchy_ok(s):
            m = Q_SCAN
        if m == Q_PAIRS:
            n, t = wq_cap(s), tri_cap(s["leaf"])
            query.append([m, s["wq_n"] * 48 + 16 * (512 + 4 * (n + t)), capped(n, s["ncap_req"]), capped(t, s["tcap_req"])])
        else:
            query.append([m, 0, 0, 0])
    e["query"] = query
    e["l2"] = list(l2_plan(s["wq_n"], s["width"], s["leaf"], s["lds_opt"], 0, 0))
    return e


# ---- the grid -------------------------------------------------------------------------------------
E1, E2, E3 = (MAX_LDS // 2 - COOP) // 48, (MAX_LDS - COOP) // 48, MAX_LDS // 48  # the LDS kernels' last fits
L2_HOST = [(n, 4, leaf, opt) for n in (1, 2, 1109, 1110, 65535) for leaf in (1, 2, 3, 4) for opt in (-1, 0, 1, 2, 10**6)] + \
          [(n, w, leaf, -1) for n, w, leaf in [(0, 4, 4), (65536, 4, 4), (100, 1, 4), (100, 5, 4), (100, 4, 5), (100, 4, 16)]]


def presence(bits):
    return dict(nodes=bits & 1, entries=bits >> 1 & 1, wq=bits >> 2 & 1, bfs=bits >> 3 & 1)


def trace_cases():
    base = dict(requested=0, n_tris=3000, cam_cap=3000, meshes=1, bounces=8, sah=100, bvh_nodes=1200, bvh_prims=2000,
                bvh_meshes=1, wq_n=800, width=4, leaf=2, node_r=0, lds_opt=-1, ncap_req=0, tcap_req=0, **presence(15))
    out = []
    # selection against the triangle counts and the images that exist
    sizes = [(12, 12), (255, 255), (256, 256), (4095, 4095), (4096, 4096), (E1, E1), (E1 + 1, 300), (E2, 5000),
             (E2 + 1, 5000), (E3, 100), (E3 + 1, 100000)]
    shapes = [(800, 2, 4, 100, 200), (2400, 2, 4, 1200, 2000), (5000, 2, 4, 3000, 5000), (100, 2, 5, 0, 0)]
    for k, meshes, bounces, bits, sah, (nt, cap), (wq_n, leaf, width, bn, bp) in itertools.product(
            range(11), (1, 64, 65), (-1, 8), (0, 1, 3, 7, 13, 15), (100, 101), sizes, shapes):
        out.append(dict(base, requested=k, meshes=meshes, bvh_meshes=meshes, bounces=bounces, sah=sah, n_tris=nt,
                        cam_cap=cap, wq_n=wq_n, leaf=leaf, width=width, bvh_nodes=bn, bvh_prims=bp,
                        node_r=(nt ^ meshes) & 1, **presence(bits)))
    # the mesh-count and bounce edges
    for k, meshes, bounces, bits, sah in itertools.product(range(11), (0, 1, 62, 63, 64, 65, 70), (-1, 0, 8), (0, 15),
                                                           (30, 500)):
        out.append(dict(base, requested=k, meshes=meshes, bvh_meshes=meshes, bounces=bounces, sah=sah, **presence(bits)))
    # the pair stacks: every 64-entry step of the node stack, the 16-bit node limit, every leaf and width, the requests
    nodes = list(range(1, 3600, 170)) + [2, 65535, 65536]
    shapes = [(leaf, 4) for leaf in range(6)] + [(2, w) for w in (1, 2, 3, 5)]
    requests = [(0, 0), (64, 0), (128, 200), (200, 128), (4096, 4096), (0, 64)]
    for k, bits, n, (leaf, width), opt, (nreq, treq) in itertools.product((AUTO, WQ, WQ_L2), (15, 7), nodes, shapes,
                                                                          (-1, 0, 2, 10**6), requests):
        out.append(dict(base, requested=k, wq_n=n, leaf=leaf, width=width, lds_opt=opt, ncap_req=nreq, tcap_req=treq,
                        node_r=n & 1, **presence(bits)))
    first_l2_host = len(out)
    for n, width, leaf, opt in L2_HOST:  # tests/test_wq_l2_host.py's cases of hrt_debug_wq_l2_plan
        out.append(dict(base, wq_n=n, width=width, leaf=leaf, lds_opt=opt))
    return out, first_l2_host


def split_cases():
    return list(itertools.product((0, 1, 30, 24575, 24576, 24577, 32400, 130000, 4000000), (0, 1, 2, 5, 20, 64),
                                  (1, 8, 256), (-1, 0, 1, 2, 3, 7)))


def build(tmp_path, extra=()):
    exe = str(tmp_path / ("launch_plan_test" + ("_san" if extra else "")))
    cmd = [os.environ.get("CXX", "c++"), "-O2", "-std=c++17", *[f"-I{d}" for d in INC], *extra, SRC, "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def run(exe):
    cases, _ = trace_cases()
    text = "".join("t " + " ".join(str(int(c[f])) for f in FIELDS) + "\n" for c in cases)
    text += "".join("s %d %d %d %d\n" % c for c in split_cases())
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_plans_match_the_rules(tmp_path):
    exe, r = build(tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    cases, first_l2_host = trace_cases()
    recs = [json.loads(line) for line in run(exe).splitlines()]
    assert len(recs) == len(cases) + len(split_cases())
    ran = set()
    for s, got in zip(cases, recs):
        assert got == expected(s), s
        k = got["kernel"]
        ran.add(k)
        # structure, whatever the rules above say
        assert got["fits"] == 1 and fits(s, k), s                 # no plan names a kernel that does not fit
        assert got["lds"] <= MAX_LDS, s
        assert all(q[1] <= MAX_LDS for q in got["query"]), s
        if s["bounces"] < 0:
            assert k == LITERAL, s
        if s["meshes"] > 64 or not s["nodes"]:
            assert k not in HIERARCHY, s
            assert all(q[0] == Q_SCAN for q in got["query"]), s
        if got["pairs"]:
            assert got["ncap"] >= 128 and got["ncap"] % 64 == 0 and got["tcap"] >= 64 and got["tcap"] % 64 == 0, s
            assert 16 * (512 + 4 * (got["ncap"] + got["tcap"])) + 48 * (got["lnodes"] if k == WQ_L2 else s["wq_n"]) <= got["lds"], s
    assert ran == set(range(1, 11))  # the grid reaches every kernel
    for (tiles, frames, cus, req), got in zip(split_cases(), recs[len(cases):]):
        waves = max(1, cus * 16 // max(1, frames))
        auto4 = 4 * (3 if tiles > 4 * waves else 1)
        if req >= 0:
            want = dict(factor=req, factor4=0, pair_factor4=4 * req, plain_factor4=4 * req)
        elif frames > 1:  # a launch of several frames splits from 1.25 x a wave's share
            want = dict(factor=req, factor4=5, pair_factor4=5, plain_factor4=auto4)
        else:
            f = 2 if tiles > 6 * cus * 16 else 3
            want = dict(factor=f, factor4=0, pair_factor4=4 * f, plain_factor4=auto4)
        assert got == dict(want, waves=waves), (tiles, frames, cus, req)
    # the library's hrt_debug_wq_l2_plan is the header's function
    lib = _lib.load()
    out = (ctypes.c_uint32 * 4)()
    for (n, width, leaf, opt), got in zip(L2_HOST, recs[first_l2_host:len(cases)]):
        lib.hrt_debug_wq_l2_plan(n, width, leaf, opt, out)
        assert list(out) == got["l2"], (n, width, leaf, opt)


def test_plans_under_sanitizers(tmp_path):
    """The same program as a stand-alone ASan + UBSan binary: no overflow, no out-of-range shift or conversion
    reported over every case, and the same output."""
    exe, r = build(tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    san, r = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    if r.returncode != 0:
        pytest.skip("the toolchain cannot link the sanitizer runtimes: " + r.stderr[-300:])
    assert run(san) == run(exe)
