"""The first-hit pass on the device (hrt_first_hits), every comparison bitwise: TILES (the
new kernel: one wave per 8x8 tile, the tile's primary triangle list) and QUERY against hrt_intersect_primary's
literal scan, in both context modes and both libraries; the statistics of counted calls, which also prove that
the path a test exists for ran; push blocks whose rays are irregular or whose counts differ from the uploaded
scene's; ordering on the context's stream and isolation from the frame loop; the rejections; the mirrors.

Sizes and paths (tools/tile_cull_model.py, the CPU restatement of the list rules, with jitter reach 0 as the pass
builds its lists): island at 130 x 70 keeps more than 64 cap survivors in 14 of its 153 tiles (the overflow
fallback beside listed tiles) and in none of the 3,600 tiles of 640 x 360 (the all-listed case); the presets' 8 x 8
image spans a cap of c_lo = 0.577, inside the rule's 0.5, so the wide-cap fallback is forced with a viewport
twice as high; a 1 x 1 image is one point with reach 0 and is listed."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from helpers import E, SceneCase, _lib
from test_gpu_intersect import degenerate, tie_soup

pytestmark = pytest.mark.gpu

SCAN = _lib.QUERY_SCAN
TILES, QUERY, AUTO = _lib.FIRST_HITS_TILES, _lib.FIRST_HITS_QUERY, _lib.FIRST_HITS_AUTO
SIZES = [(1, 1), (8, 8), (9, 9), (37, 23), (64, 64), (130, 70)]
SCENES = ["box", "spheres", "cube", "island", "cave", "ties", "degenerate"]
FILL = 0xA5
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        _hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.hipFree.argtypes = [ctypes.c_void_p]
    return _hip


class DevBuf:
    """nbytes of device memory filled with 0xA5."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        assert hip().hipMalloc(ctypes.byref(p), nbytes) == 0
        self.ptr, self.nbytes = int(p.value), nbytes
        assert hip().hipMemset(self.ptr, FILL, self.nbytes) == 0 and hip().hipDeviceSynchronize() == 0

    def read(self):
        out = np.empty(self.nbytes, np.uint8)
        assert hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return out

    def free(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = 0


@functools.lru_cache(maxsize=None)
def make_case(name, size):
    if name in ("ties", "degenerate"):
        base = tie_soup() if name == "ties" else degenerate()
        return SceneCase(settings=base.settings, camera=base.camera, size=size)
    return SceneCase(name, size, 1, 1)


def stats_tuple(st):
    return (st.method_ran, st.tiles, st.tiles_listed, st.tiles_empty, st.tiles_fallback, st.scan_rays, st.tri_tests,
            st.entries_tested)


def first_hits(ctx, pc, method, count=False, buf=None):
    """One pass into a fresh (or the given) device buffer, waited for: the bytes, and the record when counted."""
    own = buf is None
    buf = buf or DevBuf(pc.width * pc.height * 32)
    ctx.first_hits(pc, buf.ptr, method, count)
    ctx.synchronize()
    got = buf.read().tobytes()
    if own:
        buf.free()
    return (got, ctx.first_hits_stats()) if count else got


def scan_of(ctx, pc):
    hits, st = ctx.intersect_primary(pc, method=SCAN, with_stats=True)
    assert st.method_ran == SCAN
    return hits, st


def explain(got, want, width):
    g, w = (np.frombuffer(b, np.uint32).reshape(-1, 8) for b in (got, want))
    bad = np.flatnonzero((g != w).any(1))
    if bad.size == 0:
        return "identical"
    k = int(bad[0])
    return (f"{bad.size} of {len(g)} hits differ; first at pixel (x={k % width}, y={k // width}): "
            f"{np.frombuffer(got, _lib.HIT_DTYPE)[k]} vs {np.frombuffer(want, _lib.HIT_DTYPE)[k]}")


def check_both_methods(ctx, pc, want, st_scan):
    """TILES and QUERY, counted and not, against the scan's bytes and counts; -> the counted TILES record."""
    W, H = pc.width, pc.height
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    out = None
    for method in (TILES, QUERY):
        got = first_hits(ctx, pc, method)
        assert got == want, (method, explain(got, want, W))
        got, st = first_hits(ctx, pc, method, count=True)
        assert got == want, (method, "counted", explain(got, want, W))
        assert (st.method_ran, st.reserved, st.scan_rays, st.tri_tests) == (method, 0, st_scan.scan_rays, st_scan.tri_tests)
        if method == TILES:
            assert st.tiles == tiles == st.tiles_listed + st.tiles_fallback and st.tiles_empty <= st.tiles_listed
            out = st
        else:
            assert (st.tiles, st.tiles_listed, st.tiles_empty, st.tiles_fallback, st.entries_tested) == (0, 0, 0, 0, 0)
    return out


# ---- 1. both methods equal the literal scan ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def measured(name, size):
    """The scene at the size on the production library, RGBA8: the scan's bytes, and the counted TILES record
    (checked against the scan with QUERY on the way)."""
    case = make_case(name, size)
    ctx = case.context()
    hits, st_scan = scan_of(ctx, case.push())
    st = check_both_methods(ctx, case.push(), hits.tobytes(), st_scan)
    ctx.close()
    return hits, st_scan, stats_tuple(st)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_equals_scan(name, size):
    hits, st_scan, tiles_rec = measured(name, size)
    case = make_case(name, size)
    for mode, debug in ((_lib.MODE_RGBA32F, False), (_lib.MODE_RGBA8, True), (_lib.MODE_RGBA32F, True)):
        ctx = case.context(mode=mode, debug=debug)
        st = check_both_methods(ctx, case.push(), hits.tobytes(), st_scan)
        assert stats_tuple(st) == tiles_rec, (mode, debug)  # the same tiles take the same paths
        if debug:
            n, bad = ctx.check_guards()
            assert n > 0 and bad == 0
        ctx.close()


# ---- 2. the paths -----------------------------------------------------------------------------------------------

def test_island_tiles_are_listed_and_half_of_them_empty():
    hits, _, (method, tiles, listed, empty, fallback, _, _, entries) = measured("island", (640, 360))
    assert method == TILES and tiles == 3600
    assert listed > 0 and empty > 0 and fallback == 0 and entries > 0, (listed, empty, fallback, entries)
    assert (hits["kind"] == 2).any() and (hits["kind"] == 0).any()


def test_dense_tiles_overflow_beside_listed_ones():
    """island 130 x 70: 14 of the 153 tiles keep more than 64 records after the cap and the tile-corner rule
    (tools/tile_cull_model.py tile_lists, mirror arithmetic, jitter reach 0)."""
    hits, _, (_, tiles, listed, _, fallback, _, _, _) = measured("island", (130, 70))
    assert fallback > 0 and listed > 0 and listed + fallback == tiles, (listed, fallback)
    assert (hits["kind"] == 2).any()


def test_wide_cap_falls_back():
    """One 8 x 8 tile over a viewport of height 4 at focal length 1: the corner directions lie 70 degrees off the
    axis, c_lo = 0.33 < 0.5, and the tile is answered by the bundle cull."""
    _, settings = E.preset("box")
    settings.viewport_height = 4.0
    case = SceneCase(settings=settings, camera=E.preset("box")[0], size=(8, 8))
    ctx = case.context()
    hits, st_scan = scan_of(ctx, case.push())
    st = check_both_methods(ctx, case.push(), hits.tobytes(), st_scan)
    ctx.close()
    assert (st.tiles, st.tiles_fallback, st.tiles_listed, st.entries_tested) == (1, 1, 0, 0)
    assert (hits["kind"] == 2).any()


@pytest.mark.parametrize("n_meshes", [33, 12])
def test_many_meshes_fall_back(n_meshes):
    """33 one-triangle meshes: build_tile_list refuses more than 32.  12: world_hit_tile's octant word holds 8
    meshes, and the pass sends every scene above that through the bundle cull as well."""
    rng = np.random.default_rng(5)
    meshes = []
    for _ in range(n_meshes):
        v = (rng.uniform(-4, 4, 3) + rng.uniform(-1.5, 1.5, (3, 3))).astype(np.float32)
        meshes.append(E.RayTracingMesh(E.Mesh(v, np.arange(3, dtype=np.uint32)), E.LambertianMaterial([0.5, 0.5, 0.5])))
        meshes.append(E.RayTracingMesh(E.Mesh(v[::-1].copy(), np.arange(3, dtype=np.uint32)),
                                       E.LambertianMaterial([0.5, 0.5, 0.5])))
    meshes = meshes[:n_meshes]
    case = SceneCase(settings=E.RayTracerSettings(num_samples=1, max_bounces=1, use_environment_lighting=True,
                                                  mesh_data=meshes),
                     camera=E.Camera([0.0, 0.0, -12.0], [0.0, 0.0, 1.0]), size=(37, 23))
    ctx = case.context()
    hits, st_scan = scan_of(ctx, case.push())
    st = check_both_methods(ctx, case.push(), hits.tobytes(), st_scan)
    ctx.close()
    assert st.tiles_fallback == st.tiles == 15 and st.tiles_listed == 0
    assert (hits["kind"] == 2).any() and (hits["kind"] == 0).any()


# ---- 3. push blocks -----------------------------------------------------------------------------------------------

def test_push_block_counts_jitter_and_irregular_rays():
    case = make_case("box", (37, 23))
    W, H = case.size
    ctx = case.context()
    whole, _ = scan_of(ctx, case.push())
    # the push block's counts, not the uploaded ones
    fewer = case.push()
    fewer.num_spheres, fewer.num_meshes = 0, 3
    want, st_scan = scan_of(ctx, fewer)
    assert want.tobytes() != whole.tobytes() and (want["kind"] == 2).any() and not (want["kind"] == 1).any()
    check_both_methods(ctx, fewer, want.tobytes(), st_scan)
    # the jitter is no input of an un-jittered ray
    for jitter in (0.0, case.jitter, 0.5, -3.0):
        pc = case.push()
        pc.jitter_size = jitter
        for method in (TILES, QUERY):
            assert first_hits(ctx, pc, method) == whole.tobytes(), (jitter, method)
    # a zero matrix, and one with a NaN: every ray is irregular and takes the literal scan
    for entry in (0.0, float("nan")):
        pc = case.push()
        if entry == 0.0:
            pc.cam_alignment_mat[:] = [0.0] * 16
        else:
            pc.cam_alignment_mat[0] = entry
        want, st_scan = scan_of(ctx, pc)
        assert st_scan.scan_rays == W * H
        st = check_both_methods(ctx, pc, want.tobytes(), st_scan)
        assert st.scan_rays == W * H and st.entries_tested == 0
    ctx.close()


def test_camera_inside_cave():
    """The camera at the centre of cave's bounding box, which the walls enclose."""
    base = make_case("cave", (64, 64))
    a = base.tris["a"][:, :3]
    centre = (a.min(0) + a.max(0)) / 2
    case = SceneCase(settings=base.settings, camera=E.Camera([float(v) for v in centre], [0.3, -0.2, 1.0]), size=(64, 64))
    ctx = case.context()
    want, st_scan = scan_of(ctx, case.push())
    st = check_both_methods(ctx, case.push(), want.tobytes(), st_scan)
    ctx.close()
    # (the walls enclose the point, but the reference's triangles are one-sided: a fifth of the view faces it)
    assert (want["kind"] == 2).any() and (want["kind"] == 0).any() and st.tiles == 64


# ---- 4. ordering and isolation -----------------------------------------------------------------------------------------

def other_cameras(case):
    p = np.asarray(case.camera.position, np.float32)
    d = np.asarray(case.camera.direction, np.float32)
    return [E.Camera([float(v) for v in p + np.float32([0.05, 0.02, -0.03])], [float(v) for v in d + np.float32([0.0, 0.03, 0.08])]),
            E.Camera([float(v) for v in p + np.float32([-0.2, 0.1, 0.0])], [float(v) for v in d])]


def push_of(case, camera):
    moved = SceneCase(settings=case.settings, camera=camera, size=case.size)
    return moved.push()


def test_stream_order_two_cameras_repeats_and_a_new_scene():
    case = make_case("box", (37, 23))
    W, H = case.size
    ctx = case.context(debug=True)
    pcs = [case.push()] + [push_of(case, c) for c in other_cameras(case)]
    wants = [scan_of(ctx, pc)[0].tobytes() for pc in pcs]
    assert len(set(wants)) == 3
    for method in (TILES, QUERY, AUTO):
        bufs = [DevBuf(W * H * 32) for _ in pcs]
        for pc, buf in zip(pcs, bufs):  # three cameras into three buffers, one wait
            ctx.first_hits(pc, buf.ptr, method)
        ctx.synchronize()
        for buf, want in zip(bufs, wants):
            assert buf.read().tobytes() == want, (method, explain(buf.read().tobytes(), want, W))
        # the same camera again (TILES: the camera records are kept), into the same and into another buffer
        ctx.first_hits(pcs[2], bufs[2].ptr, method)
        ctx.first_hits(pcs[2], bufs[0].ptr, method)
        ctx.synchronize()
        assert bufs[2].read().tobytes() == wants[2] and bufs[0].read().tobytes() == wants[2]
        for buf in bufs:
            buf.free()
    got, st = first_hits(ctx, pcs[0], AUTO, count=True)
    assert got == wants[0] and st.method_ran in (TILES, QUERY)
    # a new scene with the same camera and mesh count: the kept records are dropped with the old scene
    assert first_hits(ctx, pcs[0], TILES) == wants[0]
    _, settings = E.preset("box")
    settings.mesh_data = [E.RayTracingMesh(E.Mesh((m.mesh.positions * np.float32(0.8)).astype(np.float32), m.mesh.indices),
                                           m.material) for m in settings.mesh_data]
    shrunk = SceneCase(settings=settings, camera=case.camera, size=case.size)
    assert len(shrunk.meshes) == len(case.meshes)
    ctx.set_scene(shrunk.rays, shrunk.spheres, shrunk.tris, shrunk.meshes)
    want = scan_of(ctx, shrunk.push())[0].tobytes()
    assert want != wants[0]
    assert first_hits(ctx, shrunk.push(), TILES) == want
    n, bad = ctx.check_guards()
    assert n > 0 and bad == 0
    ctx.close()


def _stats_tuple(st):  # (test_gpu_intersect._stats_tuple: hrt_stats without timings and wave_steps)
    return (st.segments, st.tri_tests, st.traces, st.accumulates, st.last_kernel, st.last_block, st.last_frames)


def _frame_loop(case, passes):
    """test_gpu_intersect._frame_loop with first-hit passes from other cameras in place of its queries: a 4-frame
    realtime loop over the three trace lanes and a 4-frame hrt_compute_n with fold records and a present each."""
    ctx = case.context(options={_lib.OPT_FOLD_RECORDS: 1})
    W, H = case.size
    target = DevBuf(W * H * 4)
    bufs = [DevBuf(W * H * 32) for _ in range(2)]
    pcs = [push_of(case, c) for c in other_cameras(case)] + [case.push()]
    turn = [0]

    def ask():
        if passes:
            for method in (TILES, QUERY):
                ctx.first_hits(pcs[turn[0] % 3], bufs[turn[0] % 2].ptr, method, count=turn[0] % 2 == 1)
                turn[0] += 1

    out = []
    ask()
    for k in range(4):
        ctx.trace(case.push(k))
        ask()
        ctx.accumulate(k)
        ask()
    out += [ctx.read(_lib.IMG_TRACE).tobytes(), ctx.read(_lib.IMG_ACCUM).tobytes(), _stats_tuple(ctx.stats())]
    ask()
    tickets = [ctx.present(_lib.IMG_ACCUM, target.ptr, target.nbytes, W, H)]
    ask()
    ctx.compute_n(case.push(4), 4)
    ask()
    tickets.append(ctx.present(_lib.IMG_ACCUM, target.ptr, target.nbytes, W, H))
    ask()
    ctx.present_wait(tickets[-1])
    recs, total = ctx.fold_records(with_total=True)
    out += [ctx.read(_lib.IMG_TRACE).tobytes(), ctx.read(_lib.IMG_ACCUM).tobytes(), _stats_tuple(ctx.stats()),
            recs.tobytes(), total, tickets, target.read().tobytes()]
    for b in bufs + [target]:
        b.free()
    ctx.close()
    return out


def test_passes_do_not_disturb_the_frame_loop():
    case = SceneCase("island", (64, 36), 2, 4)
    plain, mixed = _frame_loop(case, False), _frame_loop(case, True)
    names = ("trace image", "accumulator", "hrt_stats", "trace image after compute_n", "accumulator after compute_n",
             "hrt_stats after compute_n", "fold records", "fold record total", "present tickets", "presented bytes")
    for what, a, b in zip(names, plain, mixed):
        assert a == b, (what, a, b) if "hrt_stats" in what else what
    assert plain[7] >= 4 and plain[8][0] < plain[8][1]


def _chain(case, after, feed):
    """Two frames of the first view folded with counts, the first hits of both views by `feed`, hrt_reproject, a
    frame of the new view, hrt_accumulate_history, hrt_denoise guided by the new view's hits."""
    W, H = case.size
    ctx = case.context(mode=_lib.MODE_RGBA32F)
    moved = SceneCase(settings=case.settings, camera=after, size=case.size)
    hits = [DevBuf(W * H * 32), DevBuf(W * H * 32)]
    for frame in range(2):
        ctx.trace(case.push(frame))
        ctx.accumulate_history(8)
    feed(ctx, case.push(), hits[0].ptr)
    feed(ctx, moved.push(), hits[1].ptr)
    ctx.reproject(E.View(case.camera, case.size, case.settings), hits[0].ptr, E.View(after, case.size, case.settings),
                  hits[1].ptr)
    ctx.trace(moved.push(2))
    ctx.accumulate_history(8)
    out = [ctx.denoise(_lib.FMT_RGBA32F, hits[1].ptr).tobytes(), ctx.read_history().tobytes(),
           ctx.read(_lib.IMG_ACCUM, _lib.FMT_RGBA32F).tobytes(), hits[0].read().tobytes(), hits[1].read().tobytes()]
    ctx.close()
    for h in hits:
        h.free()
    return out


def test_the_four_stage_chain_fed_by_the_pass():
    case = SceneCase("box", (48, 32), 1, 2)
    after = other_cameras(case)[0]
    blocking = _chain(case, after, lambda ctx, pc, ptr: ctx.intersect_primary_into(pc, ptr))
    for method in (TILES, QUERY):
        enqueued = _chain(case, after, lambda ctx, pc, ptr: ctx.first_hits(pc, ptr, method))
        for what, a, b in zip(("denoised", "counts", "accumulator", "first view's hits", "new view's hits"), blocking, enqueued):
            assert a == b, (method, what)
    assert blocking[3] != blocking[4]  # (two views)


# ---- 5. the rejections ---------------------------------------------------------------------------------------------

def test_rejections_leave_hits_untouched():
    case = make_case("box", (37, 23))
    W, H = case.size
    buf = DevBuf(W * H * 32 + 16)
    untouched = buf.read().tobytes()
    bare = E.HrtContext(case.size, device=0)
    for method in (AUTO, TILES, QUERY):
        with pytest.raises(_lib.HrtError) as e:
            bare.first_hits(case.push(), buf.ptr, method)
        assert e.value.status == 4  # HRT_ERR_NO_SCENE
    bare.close()
    ctx = case.context()
    lib, handle = ctx.lib, ctx.handle
    got, before = first_hits(ctx, case.push(), TILES, count=True)
    host_raw = np.full(W * H * 32 + 16, 7, np.uint8)
    host_hits = host_raw.ctypes.data + (-host_raw.ctypes.data) % 16  # aligned, but pageable host memory

    def raw(pc=case.push(), method=TILES, flags=0, hits=buf.ptr):
        return lib.hrt_first_hits(handle, ctypes.byref(pc) if pc is not None else None, method, flags,
                                  ctypes.c_void_p(hits or 0))

    wrong, over, neg = case.push(), case.push(), case.push()
    wrong.width += 1
    over.num_meshes += 1
    neg.num_spheres = -1
    for kw, word in ((dict(pc=None), b"null"), (dict(hits=None), b"null"), (dict(method=3), b"method"),
                     (dict(method=0xFFFFFFFF), b"method"), (dict(flags=2), b"flag"), (dict(flags=3), b"flag"),
                     (dict(flags=0x80000000), b"flag"), (dict(hits=host_hits), b"device"), (dict(hits=buf.ptr + 8), b"aligned"),
                     (dict(pc=wrong), b"width"), (dict(pc=over), b"num_spheres/num_meshes"), (dict(pc=neg), b"num_spheres/num_meshes")):
        for method in ((kw["method"],) if "method" in kw else (AUTO, TILES, QUERY)):
            assert raw(**{**kw, "method": method}) == 1 and word in lib.hrt_last_error(handle), (kw, method)
    assert lib.hrt_get_first_hits_stats(handle, None) == 1
    # nothing ran: the buffer and the host array are as they were, the last counted record still stands
    ctx.synchronize()
    assert buf.read().tobytes() == untouched and (host_raw == 7).all()
    assert stats_tuple(ctx.first_hits_stats()) == stats_tuple(before)
    assert first_hits(ctx, case.push(), QUERY) == got  # ... and the context still works
    ctx.close()
    # the parts of a row-tile partition, and an unpartitioned context joined to a communicator
    for p in range(2):
        part = case.context(partition=(8, p, 2))
        for method in (AUTO, TILES, QUERY):
            with pytest.raises(_lib.HrtError, match="partition"):
                part.first_hits(case.push(), buf.ptr, method)
        part.close()
    single = case.context()
    E.HrtContext.comm_init_all([single])
    with pytest.raises(_lib.HrtError, match="communicator"):
        single.first_hits(case.push(), buf.ptr, TILES)
    single.close()
    assert buf.read().tobytes() == untouched
    buf.free()


# ---- 6. the mirrors -----------------------------------------------------------------------------------------------------

def test_python_and_cpp_mirrors(tmp_path):
    """RayTracePipeline.first_hits_async against first_hits_into, and include/hrt_app.hpp's first_hits_enqueue /
    Context::first_hits_stats (tests/cpp/first_hits_demo) against the Python mirror's bytes on the box scene's
    geometry."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-s", "-C", cpp, "-f", "first_hits_demo.mk"], check=True)  # (up to date after build())
    _, settings = E.preset("box")
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        f.write(np.uint32(len(settings.sphere_data)).tobytes())
        for s in settings.sphere_data:
            f.write(np.float32([*s.centre, s.radius]).tobytes())
        f.write(np.uint32(len(settings.mesh_data)).tobytes())
        for m in settings.mesh_data:
            f.write(np.uint32([len(m.mesh.positions), len(m.mesh.indices)]).tobytes())
            f.write(m.mesh.positions.tobytes())
            f.write(m.mesh.indices.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([os.path.join(cpp, "first_hits_demo"), str(src), str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    w, h = 48, 32
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [w, h] and len(raw) == 8 + 48 + 2 * w * h * 32
    demo_stats = _lib.FirstHitsStats.from_buffer_copy(raw[8:56])
    # the demo's scene through the Python mirror: the same geometry, Lambertian grey
    grey = E.LambertianMaterial([0.5, 0.5, 0.5])
    st = E.RayTracerSettings(num_samples=1, max_bounces=1, use_environment_lighting=True,
                             sphere_data=[E.Sphere(s.centre, s.radius, grey) for s in settings.sphere_data],
                             mesh_data=[E.RayTracingMesh(m.mesh, grey) for m in settings.mesh_data])
    ctx = E.HrtContext((w, h), device=0, mode=_lib.MODE_RGBA32F)
    pipe = E.RayTracePipeline(ctx, (w, h), st)
    cams = [E.Camera(), E.Camera([0.05, 0.02, -0.03], [1.0, 0.03, 0.08])]
    bufs = [DevBuf(w * h * 32), DevBuf(w * h * 32)]
    pipe.first_hits_async(cams[0], bufs[0].ptr, TILES, count=True)
    pipe.first_hits_async(cams[1], bufs[1].ptr, QUERY)
    ctx.synchronize()
    got = [b.read().tobytes() for b in bufs]
    mine = ctx.first_hits_stats()
    for cam, g in zip(cams, got):
        assert g == pipe.first_hits(cam).tobytes()
    assert got[0] != got[1] and (np.frombuffer(got[0], _lib.HIT_DTYPE)["kind"] == 2).any()
    assert raw[56:56 + w * h * 32] == got[0] and raw[56 + w * h * 32:] == got[1]
    assert stats_tuple(demo_stats) == stats_tuple(mine) and mine.method_ran == TILES and mine.tiles == 24
    for b in bufs:
        b.free()
    ctx.close()
