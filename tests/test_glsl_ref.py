"""The oracle against the reference's own shader text (CPU; DESIGN.md 2 "Parity status").

oracle/glsl_ref/ translates assets/raytracing.glsl and assets/image_combiner.glsl of the reference checkout
mechanically into C++ (into oracle/_ref/, never committed) and compiles them against a shim of the GLSL builtins
written from the numerics spec S1-S7.  Here the oracle (oracle/rt_oracle.c, a hand transliteration, and through it every
kernel test of this suite) is compared with that library: function by function on about 10^5 seeded cases plus the
edges, whole frames (texels, stored floats, triangle-test count), and the combiner on every byte pair.  Every comparison
is bitwise, two NaNs being equal (image_ref.same_floats).  The shim's own builtins are held to float64 within bounds
derived from their operation counts.  The committed digests of the shader's frames (tests/golden/glsl_ref.json) hold
the oracle to the shader in a checkout without the reference too.

tools/exp/oracle_mutant_*.patch are nine wrong oracles; DESIGN.md 2 names the test here that catches each."""
import numpy as np
import pytest

import glsl_ref_cases as G
import pyoracle
from glsl_ref_cases import unit
from helpers import E, _lib
from image_ref import assert_all_pairs, float_pool, pairs_images, same_floats, unorm8, unorm8_to_float

GLSL = pyoracle.load_glsl_ref()
needs_glsl = pytest.mark.skipif(GLSL is None, reason="no reference checkout and no built oracle/_ref/libglslref.so")

N = 100_000
SEED = 0x61F5
F32 = np.float32
U = 2.0 ** -24  # unit roundoff of binary32


def test_library_is_built_where_the_reference_exists():
    """A machine that has the reference checkout must have built and loaded the library (so the tests below cannot
    skip there), and the build's evaluation-order check holds in the loaded library."""
    if pyoracle.have_reference():
        assert GLSL is not None
    if GLSL is not None:
        assert GLSL.glr_selfcheck() == 0


TOY_SHADER = """#version 460
#define HALF 0.5
layout(local_size_x = 8, local_size_y = 8, local_size_z = 1) in;
struct Item { vec4 value; };
layout(set = 0, binding = 0, rgba8) uniform image2D target;
layout(set = 0, binding = 1) buffer Items { Item[] items; };
layout(push_constant) uniform Block { bool flip; uint count; } block;
float twice(inout uint n) { n += 1u; return 2 * HALF * n; } // a comment with 1.5 in it
void main() {
    uint k = gl_GlobalInvocationID.x;
    vec3 v = items[k].value.xyz * twice(k);
    if (block.flip) { v = -v; }
    imageStore(target, ivec2(k, 0), vec4(v, 1.0));
}
"""


def test_translator_is_mechanical_and_refuses_what_it_does_not_know():
    """oracle/glsl_ref/translate.py on a toy shader of this project's own (no reference needed): the rewrites it
    makes, and a loud stop on every construct outside them."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("glsl_translate", os.path.join(os.path.dirname(pyoracle.HERE), "oracle",
                                                                                 "glsl_ref", "translate.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    cpp = tr.translate(TOY_SHADER, "toy")
    for piece in ("#define HALF 0.5f", "thread_local image2D target;", "thread_local counted_buffer<Item> items;",
                  "bool32 flip;", "thread_local Block block;", "float twice(uint& n)", ".xyz() * twice(k)",
                  "void shader_main()", "vec4(v, 1.0f)", "namespace toy {", "2 * HALF * n"):
        assert piece in cpp, piece
    assert "comment" not in cpp and "layout" not in cpp and "#version" not in cpp
    for bad in ("vec3 v = items[k].value.xyz", "vec3 v = items[k].value.zyx"), ("2 * HALF * n", "pow(HALF, 2.0) * n"), \
            ("#define HALF 0.5", "#extension GL_foo : enable\n#define HALF 0.5"), ("vec4(v, 1.0)", "vec4(v, 1.0lf)"), \
            ("inout uint n", "out uint n"), ("void main() {", "shared float cache[64];\nvoid main() {"), \
            ("Item[] items;", "Item items[4];"), ("uniform image2D target", "uniform sampler2D target"):
        assert bad[0] in TOY_SHADER
        with pytest.raises(tr.Unknown):
            tr.translate(TOY_SHADER.replace(*bad), "toy")


# ---- helpers ---------------------------------------------------------------------------------------------------

def assert_same(x, y, what):
    if x.dtype.names:  # input records: bytes
        x, y = x.view(np.uint8), y.view(np.uint8)
    ok = same_floats(x, y) if x.dtype == F32 else (x == y)
    if not ok.all():
        bad = np.flatnonzero(~ok.reshape(-1))
        raise AssertionError(f"{what}: {bad.size} of {ok.size} values differ; first at flat index {int(bad[0])}: "
                             f"oracle {x.reshape(-1)[bad[0]]!r}, shader {y.reshape(-1)[bad[0]]!r}")


def both(name, *args):
    """Run the oracle's orc_b_<name> and the shader's glr_<name> on private copies of the arrays and demand that
    every array (outputs, RNG states) ends up the same.  Returns the oracle's arrays."""
    res = []
    for lib, prefix in ((pyoracle.load(), "orc_b_"), (GLSL, "glr_")):
        a = [x.copy() if isinstance(x, np.ndarray) else x for x in args]
        pyoracle.batch(lib, prefix + name, *a)
        res.append(a)
    for k, (x, y) in enumerate(zip(*res)):
        if isinstance(x, np.ndarray):
            assert_same(x, y, f"{name}, argument {k}")
    return res[0]


MULT_INV = pow(2654435769, -1, 2 ** 32)


def hash_inverse(h: int) -> int:
    """The state whose hash (raytracing.glsl:13-21, a bijection of uint32) is h."""
    s = (h * MULT_INV) & 0xFFFFFFFF
    s ^= s >> 16
    s = (s * MULT_INV) & 0xFFFFFFFF
    s ^= s >> 16
    s = (s * MULT_INV) & 0xFFFFFFFF
    return s ^ 2747636419


# u01 = 0, 2^-32, the words that round to u01 = 1, and u01 = 0.5 exactly (a roulette tie with a colour of 0.5)
EDGE_WORDS = [0, 1] + list(range(2 ** 32 - 128, 2 ** 32)) + [2 ** 31]


def edge_states(depth=6):
    """The edge words themselves, and the states whose k-th draw (k = 1..depth) is an edge word: log(0), u01 = 1."""
    out = list(EDGE_WORDS)
    for w in EDGE_WORDS:
        s = w
        for _ in range(depth):
            s = hash_inverse(s)
            out.append(s)
    return np.array(out, np.uint32)


def states(rng, n, depth=6):
    e = edge_states(depth)
    return np.concatenate([e, rng.integers(0, 2 ** 32, n - len(e), dtype=np.uint64).astype(np.uint32)])


def test_hash_inverse_is_the_inverse():
    for w in (0, 1, 0xFFFFFFFF, 0x12345678):
        assert pyoracle.hash_sequence(hash_inverse(w), 1) == [w]


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.0e38], F32)


def sprinkle(rng, a, fraction=0.02, pool=SPECIAL):
    """a with `fraction` of its entries replaced by special values (zeros, denormals, infinities, NaN)."""
    a = a.copy()
    hit = rng.random(a.shape) < fraction
    a[hit] = rng.choice(pool, int(hit.sum()))
    return a


def push_block(camera=None, jitter=0.0, env=1, **kw):
    case = G.scene_case("empty", (8, 8), 1, 1)
    if camera is not None:
        case.camera = camera
    pc = case.push()
    pc.jitter_size, pc.use_environment_light = float(jitter), int(env)
    for k, v in kw.items():
        setattr(pc, k, v)
    return pc


# ---- per function ----------------------------------------------------------------------------------------------

@needs_glsl
def test_rng_functions():
    """hash, scaleToRange01, RandomValueNormalDistribution, RandomPointOnUnitSphere (raytracing.glsl:13-40)."""
    rng = np.random.default_rng(SEED)
    st = states(rng, N)
    both("hash", N, st, np.zeros(N, np.uint32))
    u = both("scale01", N, st, np.zeros(N, F32))[2]
    assert u[0] == 0.0 and (u[2:130] == 1.0).all()
    nd = both("normal_dist", N, st, np.zeros(N, F32))[2]
    assert not np.isfinite(nd).all()  # log(0) was reached
    sp = both("point_on_sphere", N, st, np.zeros((N, 3), F32))[2]
    assert np.isnan(sp).any() and np.isfinite(sp).all(1).sum() > 0.99 * N


@needs_glsl
def test_point_on_hemisphere():
    """RandomPointOnHemisphere (raytracing.glsl:42-46; the shader never calls it and the oracle does not restate
    it): the unit-sphere point, negated unless its S2 dot with the normal is positive."""
    rng = np.random.default_rng(SEED + 1)
    n = 20_000
    st = states(rng, n)
    nrm = sprinkle(rng, unit(rng.normal(size=(n, 3))))
    s1, out = st.copy(), np.zeros((n, 3), F32)
    pyoracle.batch(GLSL, "glr_point_on_hemisphere", n, s1, nrm, out)
    s2, p = st.copy(), np.zeros((n, 3), F32)
    pyoracle.batch(GLSL, "glr_point_on_sphere", n, s2, p)
    d = np.zeros(n, F32)
    pyoracle.batch(GLSL, "glr_shim_op", 0, n, p, nrm, None, d)
    assert (s1 == s2).all()
    with np.errstate(invalid="ignore"):
        assert_same(np.where((d > 0)[:, None], p, -p), out, "hemisphere")


@needs_glsl
def test_get_ray_dir():
    """get_ray_dir (raytracing.glsl:162-166): three draws, u2 into the z term and u3 into the y term."""
    rng = np.random.default_rng(SEED + 2)
    cams = [E.Camera([0, 0, 0], [1, 0.5, 0.2]), E.Camera([1, 2, 3], [-0.35, -0.35, 0.87]), E.Camera([0, 1, 0], [0, -1, 0.001])]
    jitters = [0.0, 0.0123, 0.125, 1.0, 3.0e38, 1e-42, float("nan"), -0.5]
    n = N // len(jitters)
    for k, j in enumerate(jitters):
        pc = push_block(cams[k % len(cams)], jitter=j)
        cen = rng.normal(size=(n, 3)).astype(F32)
        cen[:, 0] = 1.0
        out = both("get_ray_dir", n, pc, sprinkle(rng, cen, 0.005), states(rng, n), np.zeros((n, 3), F32))[4]
        assert np.isfinite(out).any() or j != j or j > 1e30


def sphere_cases(rng, n):
    sp = np.zeros(n, _lib.SPHERE_DTYPE)
    sp["centre"] = rng.uniform(-4, 4, (n, 3))
    sp["radius"] = rng.uniform(0.05, 3, n)
    sp["material"]["colour"] = rng.random((n, 4))
    sp["material"]["settings"] = rng.random((n, 4))
    o = rng.uniform(-6, 6, (n, 3)).astype(F32)
    aim = sp["centre"] + rng.normal(size=(n, 3)) * sp["radius"][:, None] * 0.8
    d = unit(aim - o)
    # tangent rays with a discriminant of exactly 0: o = (0, r, 0), d = +z, centre (0, 0, 5), radius r (all exact)
    k = n // 20
    r = 2.0 ** rng.integers(-3, 3, k)
    sp["centre"][:k], sp["radius"][:k] = [0.0, 0.0, 5.0], r
    o[:k], d[:k] = np.stack([0 * r, r, 0 * r], -1), [0.0, 0.0, 1.0]
    # radius 0 at distance t on the ray: discriminant 0, hit distance t, with t at 0.001f and its neighbours
    t = np.array([0.001], F32).view(np.uint32)[0] + rng.integers(-2, 3, k)
    sp["centre"][k:2 * k] = 0.0
    sp["centre"][k:2 * k, 2] = t.astype(np.uint32).view(F32)
    sp["radius"][k:2 * k] = 0.0
    o[k:2 * k], d[k:2 * k] = 0.0, [0.0, 0.0, 1.0]
    sp["centre"][2 * k:3 * k] = sprinkle(rng, sp["centre"][2 * k:3 * k], 0.2)
    sp["radius"][2 * k:3 * k] = sprinkle(rng, sp["radius"][2 * k:3 * k], 0.2)
    o[3 * k:4 * k] = sprinkle(rng, o[3 * k:4 * k], 0.2)
    d[4 * k:5 * k] = sprinkle(rng, d[4 * k:5 * k], 0.2)
    return sp, o, d, k


@needs_glsl
def test_intersecting_sphere():
    """intersecting_sphere (raytracing.glsl:169-190): `discriminant >= 0`, the near root only."""
    rng = np.random.default_rng(SEED + 3)
    sp, o, d, k = sphere_cases(rng, N)
    out = both("intersecting_sphere", N, sp, o, d, np.zeros((N, 19), F32))[4]
    hit = out[:, 6] < F32(3.402823466e+38)
    assert hit[:2 * k].all(), "the zero-discriminant cases must hit"  # exact by construction
    assert 0.3 * N < hit.sum() < N


def box_cases(rng, n):
    c = rng.uniform(-3, 3, (n, 3))
    h = rng.uniform(0.01, 2, (n, 3))
    mn, mx = (c - h).astype(F32), (c + h).astype(F32)
    o = rng.uniform(-6, 6, (n, 3)).astype(F32)
    q = n // 8
    o[:q] = (c[:q] + h[:q] * rng.uniform(-1, 1, (q, 3))).astype(F32)  # inside
    face = rng.integers(0, 3, q)
    o[q:2 * q] = o[:q]
    side = np.where((rng.random(q) < 0.5)[:, None], mn[q:2 * q], mx[q:2 * q])
    o[np.arange(q, 2 * q), face] = side[np.arange(q), face]  # on a face
    d = rng.normal(size=(n, 3)).astype(F32)
    # ... and on a face with a zero direction component along that axis: 0 * inf, a NaN slab distance
    d[np.arange(q, q + q // 2), face[:q // 2]] = rng.choice(np.array([0.0, -0.0], F32), q // 2)
    o[2 * q:3 * q] = (c[2 * q:3 * q] - unit(d[2 * q:3 * q]) * 5).astype(F32)  # box behind... and ahead: flip half
    d[2 * q:2 * q + q // 2] *= -1
    zero_pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e-38, -1e-38], F32)
    d[3 * q:6 * q] = sprinkle(rng, d[3 * q:6 * q], 0.4, zero_pool)
    d[6 * q:7 * q] = sprinkle(rng, d[6 * q:7 * q], 0.2)
    o[6 * q:7 * q] = sprinkle(rng, o[6 * q:7 * q], 0.1)
    return mn, mx, o, d


@needs_glsl
def test_intersecting_aabb():
    """intersecting_aabb (raytracing.glsl:192-210) with its early returns and its min/max mix-up, on origins
    inside, on and behind the box and on zero, denormal and non-finite direction components (1 / dir infinite)."""
    rng = np.random.default_rng(SEED + 4)
    mn, mx, o, d = box_cases(rng, N)
    out = both("intersecting_aabb", N, mn, mx, o, d, np.zeros(N, np.int32))[5]
    assert 0.05 * N < out.sum() < 0.999 * N


def cross32(a, b):
    """The host's triangle normal: a.y*b.z - a.z*b.y ... in float32, no contraction."""
    a, b = a.astype(F32), b.astype(F32)
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def tri_cases(rng, n):
    t = np.zeros(n, _lib.TRIANGLE_DTYPE)
    a = rng.uniform(-3, 3, (n, 3)).astype(F32)
    e1, e2 = rng.uniform(-2, 2, (n, 3)).astype(F32), rng.uniform(-2, 2, (n, 3)).astype(F32)
    q = n // 10
    # axis-aligned triangles in the plane z = a.z, normal (0, 0, -k) exactly
    kk = (2.0 ** rng.integers(-2, 3, 3 * q)).astype(F32)
    e1[:3 * q], e2[:3 * q] = np.stack([kk, 0 * kk, 0 * kk], -1), np.stack([0 * kk, -np.ones_like(kk), 0 * kk], -1)
    e1[3 * q:4 * q] = e2[3 * q:4 * q]  # degenerate: parallel edges, zero normal
    e2[4 * q:4 * q + q // 2] = 0.0     # degenerate: a zero edge
    for name, v in (("a", a), ("edge_one", e1), ("edge_two", e2), ("normal", cross32(e1, e2))):
        t[name][:, :3], t[name][:, 3] = v, 1.0
    uv = rng.uniform(-0.2, 1.2, (n, 2))
    edge = rng.random(n) < 0.2
    uv[edge] = rng.choice([0.0, 0.5, 1.0], (int(edge.sum()), 2))  # on the edges and corners (u, v, w = 0)
    target = a + uv[:, :1] * e1 + uv[:, 1:] * e2
    o = rng.uniform(-6, 6, (n, 3)).astype(F32)
    o[:q] = target[:q].astype(F32)
    o[:q, 2] = a[:q, 2] - F32(0.001)  # axis-aligned, hit distances around 0.001
    d = (target - o).astype(F32)
    d[:q] = [0.0, 0.0, 1.0]
    d[q:q + q // 2] = e1[q:q + q // 2]          # in the triangle's plane: dot(dir, normal) exactly 0
    d[2 * q:3 * q] = unit(d[2 * q:3 * q])
    t["normal"][5 * q:6 * q, :3] = sprinkle(rng, t["normal"][5 * q:6 * q, :3], 0.2)
    o[6 * q:7 * q] = sprinkle(rng, o[6 * q:7 * q], 0.2)
    d[7 * q:8 * q] = sprinkle(rng, d[7 * q:8 * q], 0.2)
    return t, o, d, q


@needs_glsl
def test_intersecting_tri():
    """intersecting_tri (raytracing.glsl:213-241): back faces, det 0, the four sign tests, the normalised normal;
    dot(dir, normal) exactly 0, zero normals, hits on edges and corners, NaN inputs."""
    rng = np.random.default_rng(SEED + 5)
    t, o, d, q = tri_cases(rng, N)
    out = both("intersecting_tri", N, t, o, d, np.zeros((N, 4), F32))[4]
    flt_max = F32(3.402823466e+38)
    hits = out[:, 3] < flt_max
    assert 0.1 * N < hits.sum() < 0.9 * N
    assert (out[q:q + q // 2, 3] == flt_max).all() and (out[q:q + q // 2, :3] == 0).all()  # dot == 0: the first return
    assert np.isnan(out).any()


WORLD_CASES = (("box", 40_000), ("spheres", 20_000), ("island", 12_000), ("cave", 6_000), ("degenerate", 8_000),
               ("ties", 6_000), ("invisible", 8_000))


@needs_glsl
@pytest.mark.parametrize("name,n", WORLD_CASES)
def test_intersecting_mesh_and_world_hit(name, n):
    """intersecting_mesh (raytracing.glsl:243-264) per mesh and world_hit (:267-288) per scene on bounce-like rays:
    the hit record, the material picked, and the reads of the triangle buffer."""
    rng = np.random.default_rng(SEED + 6)
    case = G.scene_case(name, (16, 12), 1, 1)
    o, d = G.bounce_like_rays(case, rng, n)
    d[: n // 50] = sprinkle(rng, d[: n // 50], 0.3)
    pc = case.push()
    for m in range(len(case.meshes)):
        k = max(n // len(case.meshes), 500)
        both("intersecting_mesh", k, case.tris, case.meshes[m:m + 1], o[:k], d[:k], np.zeros((k, 19), F32), np.zeros(1, np.uint64))
    tris = case.tris if len(case.meshes) else None
    res = both("world_hit", n, pc, case.spheres if len(case.spheres) else None, tris,
               case.meshes if len(case.meshes) else None, o, d, np.zeros((n, 19), F32), np.zeros(1, np.uint64))
    hit = res[7][:, 6] < F32(3.402823466e+38)
    assert 0.2 * n < hit.sum() < n
    assert res[8][0] > 0 or not len(case.meshes)


@needs_glsl
def test_world_hit_at_exactly_a_thousandth():
    """`hit_dist > 0.001` (raytracing.glsl:251, :273, :281): a triangle and a zero-radius sphere at distances 0.001f
    and its neighbours straight ahead -- the record at exactly 0.001f must be a miss."""
    tri = np.zeros(1, _lib.TRIANGLE_DTYPE)
    bits = int(np.array([0.001], F32).view(np.uint32)[0])
    for kind in ("triangle", "sphere"):
        seen = []
        for delta in (-1, 0, 1, 2):
            t = np.array([bits + delta], np.uint32).view(F32)[0]
            case = G.scene_case("empty", (8, 8), 1, 1)
            pc = case.push()
            o, d = np.zeros((1, 3), F32), np.array([[0.0, 0.0, 1.0]], F32)
            sp = mesh = tris = None
            if kind == "triangle":
                tri["a"][0] = [-0.25, 0.25, t, 1.0]
                tri["edge_one"][0], tri["edge_two"][0], tri["normal"][0] = [1, 0, 0, 1], [0, -1, 0, 1], [0, 0, -1, 1]
                mesh = np.zeros(1, _lib.MESH_DTYPE)
                mesh["min_point"], mesh["max_point"], mesh["len"] = [-1, -1, -1], [1, 1, 1], 1
                tris, pc.num_meshes = tri, 1
            else:
                sp = np.zeros(1, _lib.SPHERE_DTYPE)
                sp["centre"][0] = [0.0, 0.0, t]
                pc.num_spheres = 1
            out = both("world_hit", 1, pc, sp, tris, mesh, o, d, np.zeros((1, 19), F32), np.zeros(1, np.uint64))[7]
            seen.append(bool(out[0, 6] == t))
        assert seen == [False, False, True, True], (kind, seen)


@needs_glsl
def test_environment_light():
    """environment_light (raytracing.glsl:290-294), switched on and off."""
    rng = np.random.default_rng(SEED + 7)
    d = sprinkle(rng, unit(rng.normal(size=(N, 3))), 0.01)
    for env in (1, 0, 2):
        out = both("environment_light", N, push_block(env=env), d, np.zeros((N, 3), F32))[3]
        assert (out != 0).any() == bool(env)


@needs_glsl
def test_adjust_dir():
    """adjust_dir (raytracing.glsl:297-305): both sphere points are always drawn; fuzz 0 and 1, metalic 0 and 1,
    specular or not; normals that are not unit, zero and NaN vectors."""
    rng = np.random.default_rng(SEED + 8)
    d, nrm = unit(rng.normal(size=(N, 3))), unit(rng.normal(size=(N, 3)))
    nrm[: N // 10] *= rng.uniform(0.5, 2.0, (N // 10, 1)).astype(F32)
    d, nrm = sprinkle(rng, d, 0.003), sprinkle(rng, nrm, 0.003)
    mats = np.zeros(N, _lib.MATERIAL_DTYPE)
    s = rng.random((N, 4)).astype(F32)
    edge = rng.random((N, 4)) < 0.5
    s[edge] = rng.choice(np.array([0.0, 1.0], F32), int(edge.sum()))
    mats["settings"] = s
    spec = rng.integers(0, 2, N).astype(np.int32)
    # reflect's factor order, I - (2 * dot(N, I)) * N: doubling is exact, so the orders differ only where 2 * dot
    # overflows and (dot * N) * 2 does not -- directions near FLT_MAX on a pure mirror
    h = N // 50
    d[:h] = (unit(rng.normal(size=(h, 3))).astype(np.float64) * 2.5e38).astype(F32)
    nrm[:h] = unit(rng.normal(size=(h, 3)))
    mats["settings"][:h], spec[:h] = [1.0, 1.0, 0.0, 0.0], 1
    out = both("adjust_dir", N, d, nrm, mats, spec, states(rng, N), np.zeros((N, 3), F32))[6]
    assert np.isfinite(out).all(1).sum() > 0.98 * N


def edge_materials(case, rng):
    """The scene's records with edge values dealt over the materials: specular probability, metalic and fuzz 0 or 1,
    the invisible flag exactly 1.0 and one ulp either side."""
    flags = np.array([0.0, 1.0, np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2))], F32)
    out = []
    for rec in (case.spheres, case.meshes):
        rec = rec.copy()
        if len(rec):
            s = rec["material"]["settings"]
            s[:, :3] = rng.choice(np.array([0.0, 1.0, 0.5], F32), (len(rec), 3))
            s[:, 3] = flags[(np.arange(len(rec)) + 1) % 4]
            rec["material"]["emission"] = rng.random((len(rec), 4)) * [1, 1, 1, 3]
            rec["material"]["colour"][:, :3] = rng.choice(np.array([0.0, 0.5, 0.9, 1.0], F32), (len(rec), 3))
        out.append(rec)
    return out


@needs_glsl
@pytest.mark.parametrize("name,n", (("box", 20_000), ("spheres", 20_000), ("invisible", 20_000), ("island", 4_000),
                                    ("ten_meshes", 3_000)))
def test_trace_ray(name, n):
    """trace_ray (raytracing.glsl:308-352) on bounce-like rays at bounce limits 0, 1 and 8, with the scene's own
    materials and with edge materials (probabilities and factors 0 and 1, roulette against a colour of 0 and of 1,
    the invisible flag at 1.0 and one ulp either side), and RNG states one of whose first 14 draws -- the 14th is the
    first bounce's roulette draw -- is 0, 0.5 or 1: `u >= p` at u == p for colours 0, 0.5 and 1."""
    rng = np.random.default_rng(SEED + 9)
    case = G.scene_case(name, (16, 12), 1, 1)
    o, d = G.bounce_like_rays(case, rng, n)
    for bounces, env, edges in ((8, 1, False), (8, 0, True), (1, 1, True), (0, 1, False)):
        spheres, meshes = edge_materials(case, rng) if edges else (case.spheres, case.meshes)
        pc = case.push()
        pc.max_bounces, pc.use_environment_light = bounces, env
        res = both("trace_ray", n, pc, spheres if len(spheres) else None, case.tris if len(meshes) else None,
                   meshes if len(meshes) else None, o, d, states(rng, n, 14), np.zeros((n, 3), F32), np.zeros(1, np.uint64))
        assert (res[8] != 0).any() or not env


# ---- whole frames ----------------------------------------------------------------------------------------------

CONFIGS = G.frame_configs()


@needs_glsl
@pytest.mark.parametrize("cfg", CONFIGS, ids=G.config_id)
def test_frame(cfg):
    """main() (raytracing.glsl:355-389) over a frame: texels, the floats handed to imageStore, and the reads of the
    triangle buffer against the oracle's rgba8, rgba32f and tri_tests."""
    case = G.case_of(cfg)
    o8, o32, seg, ott = case.oracle(want_f32=True)
    g8, g32, gtt = pyoracle.glsl_trace(case.push(), case.rays, case.spheres, case.tris, case.meshes)
    assert_same(o32, g32, "stored floats")
    assert np.array_equal(o8, g8)
    assert ott == gtt
    assert seg >= case.size[0] * case.size[1] * cfg[2]


@needs_glsl
def test_frame_configurations_cover_the_list():
    """The parameter list above, checked on the configurations themselves: every scene; spp 1 and 3; bounce limits
    0, 1 and 8; the environment on and off; rng_offset 0, 1 and 2^32 - 1; jitter 0 and huge; scenes without
    spheres, without meshes and with ten meshes; and frames in which the invisible light is hit first and after a
    visible object."""
    assert {c[0] for c in CONFIGS} == set(G.SCENES)
    assert {c[2] for c in CONFIGS} == {1, 3} and {c[3] for c in CONFIGS} == {0, 1, 8}
    assert {c[4] for c in CONFIGS} == {0, 1, 0xFFFFFFFF} and {c[5] for c in CONFIGS} == {None, True, False}
    assert {c[6] for c in CONFIGS} == {None, 0.0, 3.0e38}
    shapes = {name: G.scene_case(name, (8, 6), 1, 1) for name in ("island", "spheres", "ten_meshes", "empty")}
    assert len(shapes["island"].spheres) == 0 and len(shapes["spheres"].meshes) == 0
    assert len(shapes["ten_meshes"].meshes) >= 10 and len(shapes["empty"].meshes) == len(shapes["empty"].spheres) == 0
    # the invisible-light scene: a camera ray through the first sphere meets an invisible light first; a ray from the
    # Lambertian sphere's top meets the second one after a visible object
    case = G.scene_case("invisible", (48, 36), 3, 8)
    pc = case.push()
    o = np.array([case.camera.position, [0.0, 1.0 + 1e-3, 0.0]], F32)
    d = np.array([[0.0, -0.4 / 4.0, 1.0], [0.0, 1.0, 0.0]], F32)
    d[0] = unit(d[0])
    out = np.zeros((2, 19), F32)
    pyoracle.batch(GLSL, "glr_world_hit", 2, pc, case.spheres, case.tris, case.meshes, o, d, out, np.zeros(1, np.uint64))
    assert (out[:, 18] == 1.0).all(), out[:, 6]


@needs_glsl
def test_init_frame():
    """`init` (raytracing.glsl:363-366): opaque black, nothing traced."""
    case = G.scene_case("box", (45, 33), 3, 8)
    pc = case.push(init=True)
    o8, o32, _, ott = pyoracle.trace(pc, case.rays, case.spheres, case.tris, case.meshes, want_f32=True)
    g8, g32, gtt = pyoracle.glsl_trace(pc, case.rays, case.spheres, case.tris, case.meshes)
    assert np.array_equal(o8, g8) and (g8 == [0, 0, 0, 255]).all()
    assert_same(o32, g32, "init floats")
    assert ott == gtt == 0


@needs_glsl
def test_rows_and_pixels_entries():
    """The harness's row range and pixel list give the frame's own values (the GPU tests rely on them)."""
    case = G.scene_case("box", (45, 33), 3, 8)
    args = (case.push(), case.rays, case.spheres, case.tris, case.meshes)
    g8, g32, gtt = pyoracle.glsl_trace(*args)
    r8, r32, rtt = pyoracle.glsl_trace(*args, rows=(5, 17), nthreads=3)
    assert np.array_equal(r8[5:17], g8[5:17]) and not r8[:5].any() and not r8[17:].any()
    rng = np.random.default_rng(SEED)
    xs, ys = rng.integers(0, 45, 200), rng.integers(0, 33, 200)
    f32, u8, tests = pyoracle.glsl_trace_pixels(*args, xs, ys)
    assert_same(f32, g32[ys, xs], "pixels")
    assert np.array_equal(u8, g8[ys, xs])
    every = pyoracle.glsl_trace_pixels(*args, np.arange(45 * 33) % 45, np.arange(45 * 33) // 45)[2]
    assert int(every.sum()) == gtt and 0 < rtt < gtt


# ---- the committed digests -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", G.GOLDEN_CONFIGS, ids=G.config_id)
def test_oracle_equals_the_shader_digests(cfg):
    """The oracle's frame against the committed digests of the SHADER's frame (tests/golden/make_glsl_ref.py): never
    skipped, so a checkout without the reference still holds the oracle to the shader's text."""
    case = G.case_of(cfg)
    o8, o32, _, ott = case.oracle(want_f32=True)
    assert G.digests(o8, o32, ott) == G.golden()[G.config_id(cfg)]


@needs_glsl
@pytest.mark.parametrize("cfg", G.GOLDEN_CONFIGS, ids=G.config_id)
def test_library_equals_the_shader_digests(cfg):
    """The library built here reproduces the committed digests (the recipe, the compiler and the shim are stable)."""
    case = G.case_of(cfg)
    g8, g32, gtt = pyoracle.glsl_trace(case.push(), case.rays, case.spheres, case.tris, case.meshes)
    assert G.digests(g8, g32, gtt) == G.golden()[G.config_id(cfg)]


# ---- the combiner ----------------------------------------------------------------------------------------------

COMBINER_FRAMES = tuple(range(64)) + (254, 255, 256, 509, 510, 511, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31,
                                      2 ** 32 - 2, 2 ** 32 - 1)


@needs_glsl
def test_combiner_every_byte_pair():
    """image_combiner.glsl:22-43 against orc_accumulate_rgba8 on all 65,536 (accumulator byte, new byte) pairs of
    every colour channel, at each listed frame number.  At 2^32 - 1 the shader's `frame + 1` is a uint sum that
    wraps to 0 before its conversion to float: the division by zero S7 states."""
    acc0, new = pairs_images()
    assert_all_pairs(acc0, new)
    for frame in COMBINER_FRAMES:
        want, got = acc0.copy(), acc0.copy()
        pyoracle.accumulate_rgba8(frame, want, new)
        pyoracle.glsl_combine_rgba8(frame, got, new)
        assert np.array_equal(want, got), (frame, int((want != got).any(-1).sum()))
    last = acc0.copy()
    pyoracle.glsl_combine_rgba8(2 ** 32 - 1, last, new)
    zero = (acc0[..., :3] == 0) & (new[..., :3] == 0)
    assert (last[..., :3][zero] == 0).all() and (last[..., :3][~zero] == 255).all()  # 0/0 and x/0


# ---- the shim itself -------------------------------------------------------------------------------------------

@needs_glsl
def test_shim_builtins_against_float64():
    """dot, cross, normalize, reflect and mix against float64, with bounds from the operation counts.  u = 2^-24; a
    rounding adds at most u times the magnitude of its result; the factor 1.01 covers the second-order terms; float64
    itself adds under 1e-15 relative.  Inputs stay between 2^-10 and 2^10 in magnitude: nothing under- or overflows.
      dot      three roundings (product, fma, fma), each result at most S = sum |a_i b_i| in magnitude: 3 u S
      cross    per component two roundings, each at most T = |a_j b_k| + |a_k b_j|: 2 u T
      normalize  dot(v, v) is a sum of positive terms, relative error 3 u; sqrt halves that and rounds (1.5 u + u);
               the division rounds (u): 3.5 u relative per component
      reflect  I - (2 dot(N, I)) N per component: the dot's 3 u S doubled and scaled by |N_i|, the product's rounding
               u |2 dot N_i|, the difference's rounding u |result|
      mix      x (1 - a) + y a: (1 - a) rounds (u), both products round (u each), the sum rounds (u): at most
               u (3 |x (1 - a)| + 2 |y a|)"""
    rng = np.random.default_rng(SEED + 10)
    n = N
    mag = lambda: (rng.normal(size=(n, 3)) * 2.0 ** rng.integers(-6, 7, (n, 1))).astype(F32)  # noqa: E731
    a, b = mag(), mag()
    t = rng.uniform(-0.5, 1.5, n).astype(F32)
    A, B, T = a.astype(np.float64), b.astype(np.float64), t.astype(np.float64)
    k = 1.01 * U

    def run(op, shape):
        out = np.zeros(shape, F32)
        pyoracle.batch(GLSL, "glr_shim_op", op, n, a, b, t, out)
        return out.astype(np.float64)

    S = (np.abs(A) * np.abs(B)).sum(1)
    assert (np.abs(run(0, n) - (A * B).sum(1)) <= 3 * k * S).all()
    Tt = np.abs(np.roll(A, -1, 1) * np.roll(B, -2, 1)) + np.abs(np.roll(A, -2, 1) * np.roll(B, -1, 1))
    assert (np.abs(run(1, (n, 3)) - np.cross(A, B)) <= 2 * k * Tt).all()
    want = A / np.linalg.norm(A, axis=1, keepdims=True)
    assert (np.abs(run(2, (n, 3)) - want) <= 3.5 * k * np.abs(want)).all()
    Nn = B / np.linalg.norm(B, axis=1, keepdims=True)
    b = Nn.astype(F32)
    B = b.astype(np.float64)
    dot = (A * B).sum(1, keepdims=True)
    S = (np.abs(A) * np.abs(B)).sum(1, keepdims=True)
    want = A - 2 * dot * B
    bound = k * (6 * S * np.abs(B) + np.abs(2 * dot * B) + np.abs(want))
    assert (np.abs(run(3, (n, 3)) - want) <= bound).all()
    b = mag()
    B = b.astype(np.float64)
    want = A * (1 - T[:, None]) + B * T[:, None]
    bound = k * (3 * np.abs(A * (1 - T[:, None])) + 2 * np.abs(B * T[:, None]))
    assert (np.abs(run(4, (n, 3)) - want) <= bound).all()


@needs_glsl
def test_shim_image_store_and_load():
    """S7 on image_ref's pool of 2,060 adversarial floats: imageStore's byte, and imageLoad of every byte."""
    pool = float_pool()
    stored, loaded = np.zeros(len(pool), np.uint8), np.zeros(len(pool), F32)
    pyoracle.batch(GLSL, "glr_shim_store_load", len(pool), pool, stored, loaded)
    assert np.array_equal(stored, unorm8(pool))
    assert_same(loaded, unorm8_to_float(stored), "imageLoad")
    assert len(np.unique(stored)) == 256
