// hrt_kernels.hip -- gfx950 kernels for the path-trace dispatch (assets/raytracing.glsl).
//
// One lane per pixel; each wave owns an 8x8 pixel tile (coherent primary rays), 256-thread
// workgroups (1024 for the LDS-resident scene).  Scene records are read with wave-uniform addresses,
// so triangles stream through SGPRs and every lane tests the same triangle against its own ray.
//
// Kernel variants (hrt_option HRT_OPT_KERNEL_VARIANT, include/hip_raytrace.h), all byte-identical
// to the oracle (tests/test_gpu_parity.py):
//   LITERAL      per-sample / per-bounce loops shaped like raytracing.glsl:308-389, full test on
//                every triangle;
//   BRUTE(_LDS)  the sample and bounce loops fused into one per-lane segment loop (a lane whose path
//                ended starts its next sample), a division-free exact pre-test per triangle in two
//                wave-uniform stages; the correctly rounded 1/det path only runs when some lane may
//                accept (DESIGN.md "exact cull"); triangles via SGPRs or resident in LDS;
//   BUNDLE       primary segments (origin = cam_pos) rejected 64 triangles at a time by bounding the
//                reference's linear forms over the wave's ray directions; bounce segments deferred
//                until a wave has enough of them, then the BRUTE test;
//   BUNDLE_CULL  BUNDLE + a lane-parallel origin-box / direction-cone pre-cull for bounce segments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

#include "hip_raytrace.h"
#include "hrt_bvh.h"
#include "hrt_kernels.h"
#include "hrt_math.h"
#include "hrt_plan.h"
#include "hrt_refine.h"

namespace hrt {

#ifndef HRT_TIMELINE
#define HRT_TIMELINE 0  // per-item timeline records (tools/timeline.py; A/B builds only)
#endif
#ifndef HRT_TL_PREPASS
#define HRT_TL_PREPASS 1  // the persistent kernels' whole-tile lists built once per launch (tile_lists, r05)
#endif



// Read-only views of the uploaded std430 records.
struct Scene {
  const float4* __restrict__ rays;
  const hrt_sphere* __restrict__ spheres;
  const hrt_triangle* __restrict__ tris;
  const hrt_mesh* __restrict__ meshes;
  const float4* __restrict__ nhat;  // normalize(tri.normal) per triangle (tri_normals, same arithmetic)
};

// The kernel arguments through an opaque pointer to the kernarg segment: a field read through it is
// a scalar load at the point of use that the compiler cannot hoist out of the fused loop.  Constants
// needed only inside a phase (a bounce batch, a work item) are read this way at the phase's start, so
// they occupy SGPRs for the phase only instead of for the whole kernel (where ~120 of them were
// spilled into VGPR lanes and read back with v_readlane).
typedef const __attribute__((address_space(4))) TraceParams* KArgs;
__device__ __forceinline__ KArgs kargs() {
  KArgs p = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}
// The scene's pointers read at the point of use (shading: after a segment, not held across the loop).
__device__ __forceinline__ Scene kscene() {
  const KArgs K = kargs();
  return Scene{K->rays, K->spheres, K->tris, K->meshes, K->tri_nhat};
}

__device__ __forceinline__ f3 ld3(const float* p) { return mk(p[0], p[1], p[2]); }
__device__ __forceinline__ f3 ray_at(f3 o, f3 d, float t) { return o + d * t; }  // :158-160

// lane r's value (r < 64, every caller's index is a lane of this wave): ds_bpermute at r * 4 directly
// (__shfl's width arithmetic added the lane's 64-lane segment base: two VALU per address)
__device__ __forceinline__ uint32_t lane_read(uint32_t v, uint32_t r) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(r << 2), (int)v);
}
__device__ __forceinline__ float lane_read(float v, uint32_t r) {
  return __uint_as_float(lane_read(__float_as_uint(v), r));
}
// ray r's mesh filter (its high word only exists with more than 32 meshes)
__device__ __forceinline__ unsigned long long mask_read(unsigned long long m, uint32_t r, int meshes) {
  const uint32_t lo = lane_read((uint32_t)m, r);
  return meshes > 32 ? ((unsigned long long)lane_read((uint32_t)(m >> 32), r) << 32) | lo : lo;
}
__device__ __forceinline__ uint32_t lanes_below(unsigned long long b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}
// n + lanes_below(b), the same integer (mod 2^32): n goes in as the lane count's own addend (v_mbcnt_lo
// adds its second operand), which hipcc does not do by itself -- it counted from 0, shifted n on the
// scalar side and added both (one VALU and one SALU more per stack push)
__device__ __forceinline__ uint32_t lanes_below_from(unsigned long long b, uint32_t n) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, n));
}

// Exclusive prefix sum of x over the wave's 64 lanes in lane order, and the total (every lane active):
// a Hillis-Steele scan inside each row of 16 lanes by DPP row shifts (lanes past a row's start read 0),
// then each row adds the totals of the rows before it by the row broadcasts of lanes 15 and 31 -- six
// adds with DPP operands instead of a ballot, two lane counts and a shift per bit of x.
// The DPP form is GFX9 wave64 only (row_bcast:15/31 do not exist on GFX10+) and needs every lane active
// (an inactive lane's row sum would be missing from the broadcast): other targets take the ballot scan,
// and HRT_KERNEL_ASSERTS=1 builds check the exec mask on entry.
#ifndef HRT_DPP_SCAN
#define HRT_DPP_SCAN 1
#endif
#ifndef HRT_KERNEL_ASSERTS
#define HRT_KERNEL_ASSERTS 0
#endif
__device__ __forceinline__ uint32_t wave_scan_excl(uint32_t x, uint32_t& total, uint32_t bits = 32u) {
#if HRT_KERNEL_ASSERTS
  if (__builtin_amdgcn_read_exec() != ~0ull) __builtin_trap();
#endif
#if HRT_DPP_SCAN && (defined(__GFX9__) || !defined(__HIP_DEVICE_COMPILE__))
  (void)bits;
  // (inline: hipcc left each __builtin_amdgcn_mov_dpp as a separate move before a plain add.  Each step
  // reads the previous one's result through DPP, which needs two wait states after a VALU write: the
  // s_nops; in place, so the rows a broadcast's row mask leaves unwritten keep their value, i.e. add 0)
  uint32_t v = x;
  asm volatile(
      "s_nop 1\n"
      "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
      "s_nop 1\n"
      "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
      "s_nop 1\n"
      "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
      "s_nop 1\n"
      "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
      "s_nop 1\n"
      "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n"
      "s_nop 1\n"
      "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n"
      "s_nop 1\n"
      : "+v"(v));
  total = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
  return v - x;
#else
  // bit-plane ballots: x < 2^bits
  uint32_t pos = 0;
  total = 0;
  for (uint32_t b = 0; b < bits; ++b) {
    const unsigned long long bb = __ballot((x >> b) & 1u);
    pos += lanes_below(bb) << b;
    total += (uint32_t)__popcll(bb) << b;
  }
  return pos;
#endif
}

// Cross-lane handoffs through LDS (the pair stacks, the closest-hit slots, the band marks).  A lane's
// store read by ANOTHER lane is a data exchange between threads, so it is written as one: relaxed
// wavefront-scope atomics for the exchanged words and a wavefront-scope acquire-release fence between
// every producer and its consumers (wave_handoff).  On gfx950 these compile to the plain ds_read /
// ds_write and no instruction at all -- a wave's LDS accesses complete in program order -- but they
// stop the compiler from reasoning per lane: with plain accesses it may forward a lane's own store to
// its later load of the same word or move a load above another lane's store (r03: that forwarding lost
// the band marks of lists starting at a lane with no list; tests/test_gpu_boundary.py's protocol tests
// run these helpers through hrt_debug_wq_protocol).
template <class T>
__device__ __forceinline__ void lds_put(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
template <class T>
__device__ __forceinline__ T lds_get(const T* p) {
  return __hip_atomic_load(const_cast<T*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
#ifndef HRT_WQ_HANDOFF
#define HRT_WQ_HANDOFF 1
#endif
__device__ __forceinline__ void wave_handoff() {
#if HRT_WQ_HANDOFF
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#endif
}

// local (compacted) row -> global row, hrt_create_info partition.
__device__ __forceinline__ uint32_t global_row(uint32_t lr, const TraceParams& /*P*/) {
  const KArgs K = kargs();  // (once per work item)
  const uint32_t parts = K->part_count, rt = K->row_tile;
  if (parts <= 1) return lr;
  const uint32_t tile = lr / rt, r = lr - tile * rt;
  return (tile * parts + K->part_index) * rt + r;
}

// get_ray_dir, raytracing.glsl:162-166 (u1, u2, u3 in that order)
template <class PC>
__device__ __forceinline__ f3 get_ray_dir(const PC& pc, f3 c, uint32_t& state) {
  // (u01 * 2) * pi: the doubling is exact too, so one multiply by pi 2^-31 (u01_mul)
  const float r = u01_mul(hash(state), 3.14159265358979323846f * 0x1p-31f);
  float sr, cr;
  spec_sincos_angle(r, sr, cr);  // r in [0, 2pi]
  // (r03, measured slower: the zero components of t1 / t2 as signed zeros -- 4.5 M fewer VALU per
  // frame, 2.150 -> 2.163 ms -- and the second normalize's sqrt and reciprocal from the bits of
  // |a|^2 near 1 -- 9 M more, 2.161 ms; profiles/r03/r03p_raygen_ab.jsonl)
  const float j = pc.jitter_size;
  const float s2 = sqrt_rng(u01(hash(state)));
  const f3 t1 = ((mk(0.0f, 0.0f, 1.0f) * cr) * j) * s2;
  const float s3 = sqrt_rng(u01(hash(state)));
  const f3 t2 = ((mk(0.0f, 1.0f, 0.0f) * sr) * j) * s3;
  const f3 nc = (c + t1) + t2;
  const auto& M = pc.cam_alignment_mat;
  const f3 w = mk(__builtin_fmaf(M[8], nc.z, __builtin_fmaf(M[4], nc.y, M[0] * nc.x)),
                  __builtin_fmaf(M[9], nc.z, __builtin_fmaf(M[5], nc.y, M[1] * nc.x)),
                  __builtin_fmaf(M[10], nc.z, __builtin_fmaf(M[6], nc.y, M[2] * nc.x)));
  return normalize_fl(w);
}
#ifndef HRT_NORM_UNIFORM
#define HRT_NORM_UNIFORM 1  // (r04b: with HRT_SKY_ZERO island 1.903 -> 1.876 ms per frame)
#endif
#ifndef HRT_SKY_ZERO
#define HRT_SKY_ZERO 1
#endif
// get_ray_dir for the sky loop (all 64 lanes run it).  Zero: the caller has checked, for the whole
// item, that jitter_size is finite and every active lane's centre has finite c.x != 0 and c.y != 0.  Then the
// zero components of t1 = ((0, 0, 1) cr j) s2 and t2 = ((0, 1, 0) sr j) s3 are signed zeros (cr, sr,
// s2, s3 are finite, s2, s3 >= +0), c.x + t1.x + t2.x == c.x and c.y + t1.y == c.y exactly, and only
// t2.z's sign can matter (when c.z + t1.z is a zero): sign(sr) ^ sign(j).  The same bits as
// get_ray_dir with 8 fewer VALU.
template <bool Zero, class PC>
__device__ __forceinline__ f3 get_ray_dir_sky(const PC& pc, f3 c, uint32_t& state) {
  if constexpr (!Zero) {
#if HRT_NORM_UNIFORM
    const float r = u01_mul(hash(state), 3.14159265358979323846f * 0x1p-31f);  // (u01 * 2) * pi
    float sr, cr;
    spec_sincos_angle(r, sr, cr);
    const float j = pc.jitter_size;
    const float s2 = sqrt_rng(u01(hash(state)));
    const f3 t1 = ((mk(0.0f, 0.0f, 1.0f) * cr) * j) * s2;
    const float s3 = sqrt_rng(u01(hash(state)));
    const f3 t2 = ((mk(0.0f, 1.0f, 0.0f) * sr) * j) * s3;
    const f3 nc = (c + t1) + t2;
    const auto& M = pc.cam_alignment_mat;
    return normalize_wu(mk(__builtin_fmaf(M[8], nc.z, __builtin_fmaf(M[4], nc.y, M[0] * nc.x)),
                           __builtin_fmaf(M[9], nc.z, __builtin_fmaf(M[5], nc.y, M[1] * nc.x)),
                           __builtin_fmaf(M[10], nc.z, __builtin_fmaf(M[6], nc.y, M[2] * nc.x))));
#else
    return get_ray_dir(pc, c, state);
#endif
  } else {
    const float r = u01_mul(hash(state), 3.14159265358979323846f * 0x1p-31f);  // (u01 * 2) * pi
    float sr, cr;
    spec_sincos_angle(r, sr, cr);
    const float j = pc.jitter_size;
    const float s2 = sqrt_rng(u01(hash(state)));
    const float t1z = (cr * j) * s2;  // ((1 cr) j) s2
    const float s3 = sqrt_rng(u01(hash(state)));
    const float t2y = (sr * j) * s3;
    const float z2 = bitsf((fbits(sr) ^ fbits(j)) & 0x80000000u);  // t2.z = ((0 sr) j) s3
    const f3 nc = mk(c.x, c.y + t2y, (c.z + t1z) + z2);
    const auto& M = pc.cam_alignment_mat;
    const f3 w = mk(__builtin_fmaf(M[8], nc.z, __builtin_fmaf(M[4], nc.y, M[0] * nc.x)),
                    __builtin_fmaf(M[9], nc.z, __builtin_fmaf(M[5], nc.y, M[1] * nc.x)),
                    __builtin_fmaf(M[10], nc.z, __builtin_fmaf(M[6], nc.y, M[2] * nc.x)));
    return HRT_NORM_UNIFORM ? normalize_wu(w) : normalize(w);
  }
}

// intersecting_aabb, raytracing.glsl:192-210, restated with its min/max quirks (:202, :206); inv =
// (1/d.x, 1/d.y, 1/d.z) correctly rounded (computed once per ray for all meshes).
__device__ __forceinline__ bool aabb_pass_inv(const hrt_mesh& m, f3 o, f3 inv) {
  float d_max = (((inv.x < 0.0f) ? m.min_point[0] : m.max_point[0]) - o.x) * inv.x;
  float d_min = (((inv.x < 0.0f) ? m.max_point[0] : m.min_point[0]) - o.x) * inv.x;
  if (d_max > 0.0f || d_min > 0.0f) return true;
  d_max = gmax(d_max, (((inv.y < 0.0f) ? m.min_point[1] : m.max_point[1]) - o.y) * inv.y);
  d_min = gmin(d_max, (((inv.y < 0.0f) ? m.max_point[1] : m.min_point[1]) - o.y) * inv.y);
  if (d_max > 0.0f || d_min > 0.0f) return true;
  d_max = gmax(d_max, (((inv.z < 0.0f) ? m.min_point[2] : m.max_point[2]) - o.z) * inv.z);
  d_min = gmax(d_min, (((inv.z < 0.0f) ? m.max_point[2] : m.min_point[2]) - o.z) * inv.z);
  return d_max > 0.0f || d_min > 0.0f;
}
__device__ __forceinline__ bool aabb_pass(const hrt_mesh& m, f3 o, f3 d) {
  return aabb_pass_inv(m, o, mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z));
}

// Result of world_hit: closest distance and what produced it (kind 0 none, 1 sphere, 2 triangle).
struct Closest {
  float t;
  int kind;
  uint32_t idx;   // sphere index or triangle index
  uint32_t mesh;  // mesh index (kind 2)
};

// intersecting_sphere, raytracing.glsl:169-190; returns dist or FLT_MAX (miss).
__device__ __forceinline__ float sphere_dist(const hrt_sphere& s, f3 o, f3 d) {
  const f3 l = o - ld3(s.centre);
  const float a = dot(d, d);
  const float half_b = dot(d, l);
  const float c = dot(l, l) - s.radius * s.radius;
  const float disc = half_b * half_b - a * c;
  if (disc >= 0.0f) return (-half_b - __builtin_sqrtf(disc)) / a;
  return kFltMax;
}

// Exact intersecting_tri (raytracing.glsl:213-241) acceptance against a running closest t:
// true iff the reference returns a hit with 0.001 < dist < best (every early return is a miss).
__device__ __forceinline__ bool tri_accept_exact(const hrt_triangle& tri, f3 o, f3 d, float best, float& t_out) {
  const f3 n = ld3(tri.normal);
  const float dn = dot(d, n);
  const f3 ao = o - ld3(tri.a);
  const f3 dao = cross(ao, d);
  const float det = -dn;
  const float inv_det = 1.0f / det;
  const float dist = dot(ao, n) * inv_det;
  const float u = dot(ld3(tri.edge_two), dao) * inv_det;
  const float v = -dot(ld3(tri.edge_one), dao) * inv_det;
  const float w = 1.0f - u - v;
  t_out = dist;
  return !(dn >= 0.0f) && !(det == 0.0f) && !(dist < 0.0f) && !(u < 0.0f) && !(v < 0.0f) && !(w < 0.0f) &&
         dist > 0.001f && dist < best;
}

// world_hit, raytracing.glsl:267-288.  Spheres first, then meshes, strict '<' against one running
// closest (equivalent to the reference's per-mesh closest + world compare: the first triangle in
// buffer order attaining the minimum wins either way).
__device__ __forceinline__ Closest world_hit_literal(const Scene& sc, const hrt_push_constants& pc, f3 o, f3 d,
                                                     uint32_t& tests) {
  Closest c{kFltMax, 0, 0u, 0u};
  for (int i = 0; i < pc.num_spheres; ++i) {
    const float t = sphere_dist(sc.spheres[i], o, d);
    if (t > 0.001f && t < c.t) c = Closest{t, 1, (uint32_t)i, 0u};
  }
  for (int m = 0; m < pc.num_meshes; ++m) {
    const hrt_mesh& mesh = sc.meshes[m];
    if (!aabb_pass(mesh, o, d)) continue;
    tests += mesh.len;
    const uint32_t end = mesh.first_index + mesh.len;
    for (uint32_t i = mesh.first_index; i < end; ++i) {
      float t;
      if (tri_accept_exact(sc.tris[i], o, d, c.t, t)) c = Closest{t, 2, i, (uint32_t)m};
    }
  }
  return c;
}

struct HitRecord {
  f3 normal, pos;
  const hrt_material* mat;
};

__device__ __forceinline__ HitRecord resolve_hit(const Scene& sc, const Closest& c, f3 o, f3 d) {
  HitRecord h;
  h.pos = ray_at(o, d, c.t);
  if (c.kind == 1) {
    const hrt_sphere& s = sc.spheres[c.idx];
    h.normal = normalize(h.pos - ld3(s.centre));
    h.mat = &s.material;
  } else {
    const float4 nh = sc.nhat[c.idx];  // = normalize(ld3(sc.tris[c.idx].normal)), computed once per scene
    h.normal = mk(nh.x, nh.y, nh.z);
    h.mat = &sc.meshes[c.mesh].material;
  }
  return h;
}

// environment_light, raytracing.glsl:290-294
template <class PC>
__device__ __forceinline__ f3 environment_light(const PC& pc, f3 d) {
  if (!pc.use_environment_light) return mk(0.0f, 0.0f, 0.0f);
  const float a = 0.5f * (d.y + 1.0f);
  const float oma = 1.0f - a;
  return mk(oma * 1.0f + a * 0.5f, oma * 1.0f + a * 0.7f, oma * 1.0f + a * 1.0f);
}

// adjust_dir, raytracing.glsl:297-305 (both unit-sphere draws always happen: 12 hashes)
#ifndef HRT_FUZZ_FAST
#define HRT_FUZZ_FAST 1
#endif
#ifndef HRT_FUZZ_INT
#define HRT_FUZZ_INT 1  // the fast path's radius test on the hash bits (r03ai)
#endif
__device__ __forceinline__ f3 adjust_dir(f3 d, f3 n, const hrt_material& mat, bool specular, uint32_t& state) {
  const f3 diffuse_dir = normalize_fl(n + unit_sphere(state));
  const float k = 2.0f * dot(n, d);
  const f3 specular_dir = d - n * k;
  const float a = mat.settings[1] * (float)(int)specular;
  const float oma = 1.0f - a;
#if HRT_FUZZ_FAST
  // Without fuzz and specular blend (settings[2] == +-0, a == +-0: a Lambertian hit), mixed + fuzz is
  // diffuse_dir * 1 + specular_dir * (+-0) + unit_sphere * (+-0) component by component, i.e.
  // diffuse_dir itself when each of its components is finite and nonzero (adding a signed zero keeps
  // it), specular_dir is finite, and the fuzz draw is finite: each of its three normal_dist radii
  // sqrt(-2 log u) is finite and nonzero exactly when u01 of its second hash is neither 0 nor 1
  // (spec_log(1) = +0, spec_log(0) = -inf; cos of the angle is never 0, hrt_math.h), so its length
  // is not 0.  Such a lane only advances the RNG by the draw's six hashes.
  const float fz = mat.settings[2];
  uint32_t st = state;
  bool fast = a == 0.0f && fz == 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    hash(st);  // the angle's
#if HRT_FUZZ_INT
    // u01(h) = RN(h) 2^-32 is 0 iff h == 0 and 1 iff RN(h) == 2^32, i.e. h >= 2^32 - 128 (the u32 -> f32
    // conversion rounds to nearest even: 2^32 - 128 is a tie between 2^32 - 256 (odd) and 2^32), so
    // the radius test is one integer compare instead of a conversion, a multiply and two compares
    fast &= hash(st) - 1u < 0xFFFFFF7Fu;
#else
    const float u = u01(hash(st));
    fast &= u != 0.0f && u != 1.0f;
#endif
  }
  const bool finite_nz = fabsf(diffuse_dir.x) < __builtin_inff() && fabsf(diffuse_dir.y) < __builtin_inff() &&
                         fabsf(diffuse_dir.z) < __builtin_inff() && diffuse_dir.x != 0.0f && diffuse_dir.y != 0.0f &&
                         diffuse_dir.z != 0.0f;
  const bool spec_ok = fabsf(specular_dir.x) < __builtin_inff() && fabsf(specular_dir.y) < __builtin_inff() &&
                       fabsf(specular_dir.z) < __builtin_inff();
  if (fast && finite_nz && spec_ok) {
    state = st;
    return normalize_fl(diffuse_dir);
  }
#endif
  const f3 fuzz = unit_sphere(state) * mat.settings[2];
  const f3 mixed = mk(diffuse_dir.x * oma + specular_dir.x * a, diffuse_dir.y * oma + specular_dir.y * a,
                      diffuse_dir.z * oma + specular_dir.z * a);
  return normalize_fl(mixed + fuzz);
}

// Per-lane path state of trace_ray (raytracing.glsl:308-352).
struct Path {
  f3 light, colour, pos, dir;
  int bounce;       // loop index i of :316
  bool not_visible; // has_not_hit_visible_object
};

// One iteration of trace_ray's loop body after world_hit (:318-346).  Returns true when the path
// has ended (break); the caller then adds light*colour.
__device__ __forceinline__ bool shade_step(const Scene& sc, const hrt_push_constants& pc, Path& p, const Closest& c,
                                           uint32_t& state) {
  if (c.kind != 0) {  // hit.hit_dist < FLT_MAX
    const HitRecord hit = resolve_hit(sc, c, p.pos, p.dir);
    const hrt_material& m = *hit.mat;
    const bool invis = (m.settings[3] == 1.0f);
    p.pos = adds(hit.pos, (float)(int)invis * 0.001f);
    if (invis && p.not_visible) {
      p.pos = hit.pos + p.dir * 0.001f;
      return false;  // continue
    }
    p.not_visible = false;
    const bool is_spec = u01(hash(state)) < m.settings[0];
    p.dir = adjust_dir(p.dir, hit.normal, m, is_spec, state);
    const f3 emitted = ld3(m.emission) * m.emission[3];
    p.light = p.light + emitted * p.colour;
    p.colour = p.colour * ld3(m.colour);
    const float prob = gmax(p.colour.x, gmax(p.colour.y, p.colour.z));
    if (u01(hash(state)) >= prob) return true;
    p.colour = div3(p.colour, prob);
    return false;
  }
  p.light = p.light + environment_light(pc, p.dir);
  return true;
}

// shade_step in two phases (trace_fused_split).  Of a hit's shading only the new
// direction is not needed at once: a lane that survives waits for its wave's next bounce batch, and a
// lane that the roulette or the bounce limit ends never reads it.  shade_hit (phase A, at the hit) is
// shade_step without adjust_dir: p.pos, emission, p.colour, the roulette on the RNG state after the
// hit's 14 hashes (is_spec's, adjust_dir's 6 + 6 in either of its arms, the roulette's) -- none of
// which depends on the direction.  A surviving hit keeps its old p.dir and leaves a Pending record;
// shade_dir (phase B, once per bounce batch, all of the batch's lanes together) fetches the normal and
// the material again and runs adjust_dir on the same inputs from the same RNG state.  normalize_fl
// gives the same bits whichever lanes share the wave (hrt_math.h), so the direction is the one
// shade_step computes.
#ifndef HRT_SHADE_PREDRAW
#define HRT_SHADE_PREDRAW 0  // 1: the RNG state before the draw in a VGPR of its own; 0: re-advanced in phase B
#endif
// The hit that owes a direction.  Packed (the pair-traversal kernels: a hierarchy exists, so at most 64
// meshes and 2^26 - 1 triangles): a triangle as (mesh << 26 | triangle) + 1 in one register, as the
// traversal's slots hold it; the capped kernels have no second VGPR to give without a scratch access in
// the fused loop.  sphere is a lane mask, not a VGPR.
template <bool Packed>
struct Pending {
  uint32_t id = 0;      // triangle (see above) or sphere index + 1; 0: nothing pending
  uint32_t mesh = 0;    // the triangle's mesh (dead when Packed)
  bool sphere = false;  // id is a sphere's
#if HRT_SHADE_PREDRAW
  uint32_t st = 0;  // state after is_spec's hash
#endif
  __device__ __forceinline__ uint32_t tri() const { return Packed ? (id - 1u) & 0x3FFFFFFu : id - 1u; }
  __device__ __forceinline__ uint32_t mesh_of() const { return Packed ? (id - 1u) >> 26 : mesh; }
};

// Phase A.  last: this segment is the path's last allowed one (its new direction would be dead too).
// Returns true when the path has ended, as shade_step does.  With HRT_SHADE_PREDRAW 0 a lane with a
// pending direction keeps the state from before the hit, and phase B advances it by the 14 hashes.
// A sphere's normal comes from the hit position BEFORE the invisible-light offset (which turns -0 into
// +0 even when it adds nothing), so a sphere hit with a pending direction keeps that position in p.pos
// and phase B applies the offset after the normal; nothing reads p.pos in between.
template <bool Packed>
__device__ __forceinline__ bool shade_hit(const Scene& sc, const hrt_push_constants& pc, Path& p, const Closest& c,
                                          uint32_t& state, bool last, Pending<Packed>& pd) {
  if (c.kind != 0) {
    const bool sph = c.kind == 1;
    const f3 hpos = ray_at(p.pos, p.dir, c.t);
    const hrt_material& m = sph ? sc.spheres[c.idx].material : sc.meshes[c.mesh].material;
    const bool invis = (m.settings[3] == 1.0f);
    p.pos = adds(hpos, (float)(int)invis * 0.001f);
    if (invis && p.not_visible) {
      p.pos = hpos + p.dir * 0.001f;
      return false;  // continue: a waiting lane with nothing pending
    }
    p.not_visible = false;
    uint32_t st = state;
    const uint32_t s1 = hash(st);  // is_spec's
#pragma unroll
    for (int k = 0; k < 12; ++k) hash(st);  // adjust_dir's two draws
    const f3 emitted = ld3(m.emission) * m.emission[3];
    p.light = p.light + emitted * p.colour;
    p.colour = p.colour * ld3(m.colour);
    const float prob = gmax(p.colour.x, gmax(p.colour.y, p.colour.z));
    if (u01(hash(st)) >= prob) {
      state = st;
      return true;
    }
    p.colour = div3(p.colour, prob);
    if (last) {
      state = st;
      return false;
    }
    if (sph) p.pos = hpos;
    pd.id = (Packed && !sph ? (c.mesh << 26) | c.idx : c.idx) + 1u;
    pd.mesh = c.mesh;
    pd.sphere = sph;
#if HRT_SHADE_PREDRAW
    pd.st = s1;
    state = st;
#else
    (void)s1;
#endif
    return false;
  }
  p.light = p.light + environment_light(pc, p.dir);
  return true;
}

// Phase B, for the lanes of a bounce batch with a pending direction.
template <bool Packed>
__device__ __forceinline__ void shade_dir(const Scene& sc, Path& p, uint32_t& state, Pending<Packed>& pd) {
  f3 n;
  const hrt_material* mat;
  if (pd.sphere) {
    const hrt_sphere& s = sc.spheres[pd.id - 1u];
    n = normalize(p.pos - ld3(s.centre));  // resolve_hit's
    mat = &s.material;
    p.pos = adds(p.pos, (float)(int)(s.material.settings[3] == 1.0f) * 0.001f);
  } else {
    const float4 nh = sc.nhat[pd.tri()];
    n = mk(nh.x, nh.y, nh.z);
    mat = &sc.meshes[pd.mesh_of()].material;
  }
  const hrt_material& m = *mat;
#if HRT_SHADE_PREDRAW
  uint32_t st = pd.st;
  const bool is_spec = u01(st) < m.settings[0];
  p.dir = adjust_dir(p.dir, n, m, is_spec, st);
#else
  const bool is_spec = u01(hash(state)) < m.settings[0];
  p.dir = adjust_dir(p.dir, n, m, is_spec, state);
  hash(state);  // the roulette's
#endif
  pd.id = 0u;
}

__device__ __forceinline__ void store_pixel(const TraceParams& /*P*/, uint32_t x, uint32_t lr, f3 col,
                                            uint32_t frame = 0) {
  const KArgs K = kargs();  // (once per work item)
  const size_t idx = (size_t)lr * K->pc.width + x + frame * K->frame_stride;
  uint32_t* img8 = K->img8;
  float4* img32 = K->img32;
  if (img8) img8[idx] = unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | (255u << 24);
  if (img32) img32[idx] = make_float4(col.x, col.y, col.z, 1.0f);
}

// wave-level sums of the per-lane counters (+ the wave's longest lane), in every lane.
__device__ __forceinline__ void wave_counters(uint32_t segs, uint32_t tests, unsigned long long& s,
                                              unsigned long long& t, uint32_t& mx) {
  s = segs;
  t = tests;
  mx = segs;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    t += __shfl_xor(t, off, 64);
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
  }
}
__device__ __forceinline__ void add_counters(const TraceParams& /*P*/, unsigned long long s, unsigned long long t,
                                             unsigned long long mx) {
  unsigned long long* counters = kargs()->counters;
  if (counters && (threadIdx.x & 63) == 0) {
    atomicAdd(&counters[0], s);
    atomicAdd(&counters[1], t);
    atomicAdd(&counters[2], mx);
  }
}
// one atomic each per wave
__device__ __forceinline__ void flush_counters(const TraceParams& P, uint32_t segs, uint32_t tests) {
  if (!kargs()->counters) return;
  unsigned long long s, t;
  uint32_t mx;
  wave_counters(segs, tests, s, t, mx);
  add_counters(P, s, t, mx);
}

__device__ __forceinline__ void lane_pixel(const TraceParams& P, uint32_t& x, uint32_t& lr) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  lr = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
}

// ---- literal variant: raytracing.glsl main (:355-389) with trace_ray's loop as written ----------
__global__ __launch_bounds__(256) void trace_literal(TraceParams P) {
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  const hrt_push_constants& pc = P.pc;
  uint32_t x, lr;
  lane_pixel(P, x, lr);
  const uint32_t y = global_row(lr, P);
  uint32_t segs = 0, tests = 0;
  if (x < pc.width && lr < P.local_rows && y < pc.height) {
    const uint32_t id = x + y * pc.width;
    f3 colour = mk(0.0f, 0.0f, 0.0f);
    uint32_t state = pc.rng_offset * 719393u + id;
    const float4 rc = sc.rays[id];
    const f3 centre = mk(rc.x, rc.y, rc.z);
    const f3 root = mk(pc.cam_pos[0], pc.cam_pos[1], pc.cam_pos[2]);
    for (int s = 0; s < pc.num_samples; ++s) {
      const f3 dir = get_ray_dir(pc, centre, state);
      Path p{mk(0.0f, 0.0f, 0.0f), mk(1.0f, 1.0f, 1.0f), root, normalize(dir), 0, true};
      for (int i = 0; i <= pc.max_bounces; ++i) {
        const Closest c = world_hit_literal(sc, pc, p.pos, p.dir, tests);
        ++segs;
        if (shade_step(sc, pc, p, c, state)) break;
      }
      colour = colour + p.light * p.colour;
    }
    colour = div3(colour, (float)pc.num_samples);
    store_pixel(P, x, lr, colour);
  }
  flush_counters(P, segs, tests);
}

// ---- exact pre-test shared by the tuned variants ----------------------------------------------------
//
// Exact cull (proof in DESIGN.md): with det = -dot(d,n) > 0 and inv = RN(1/det) > 0, the reference
// can only accept a triangle if none of these division-free rejections holds (when det >= 2^-60):
//   R6  num_t <  RN(det * 0.000999)           (then dist < 0.001)
//   R3  num_u < -RN(det * 2^-60)              (then u = RN(num_u*inv) < 0, no underflow to -0)
//   R4  num_v >  RN(det * 2^-60)              (then v < 0)
//   R5  RN(num_u - num_v) > RN(det * (1+2^-16))   (then w = 1-u-v < 0)
//   R7  num_t >  RN(best_k * det), best_k = RN(best * (1+2^-16))   (then dist > best)
// A lane that passes the pre-test is only a candidate; the exact reference expression decides.
constexpr float kTiny = 8.673617379884035e-19f;   // 2^-60
constexpr float kOnePlus = 1.0000152587890625f;   // 1 + 2^-16
constexpr float kTMin = 0.000999f;

// Division-free quantities of one triangle test, computed exactly as the reference does.
struct TriPre {
  float num_t, num_u, num_v, det;
  bool cand;
};

__device__ __forceinline__ bool pre_reject(const TriPre& q, float best_k) {
  const float tiny = q.det * kTiny;
  const bool r = (q.num_t < q.det * kTMin) | (q.num_u < -tiny) | (q.num_v > tiny) |
                 ((q.num_u - q.num_v) > q.det * kOnePlus) | (q.num_t > best_k * q.det);
  return r & !(q.det < kTiny);
}

// The reference's remaining arithmetic (raytracing.glsl:227-238) for a candidate lane.
__device__ __forceinline__ void tri_exact(const TriPre& q, uint32_t i, uint32_t m, Closest& c, float& best_k) {
  const float inv_det = 1.0f / q.det;
  const float dist = q.num_t * inv_det;
  const float u = q.num_u * inv_det;
  const float v = -q.num_v * inv_det;
  const float w = 1.0f - u - v;
  if (!(dist < 0.0f) && !(u < 0.0f) && !(v < 0.0f) && !(w < 0.0f) && dist > 0.001f && dist < c.t) {
    c = Closest{dist, 2, i, m};
    best_k = dist * kOnePlus;
  }
}

// Two-stage test of one triangle record (a, e1, e2, n as float4 with unused w): stage 1 computes
// ao and num_t and leaves when no lane has num_t > 0 (necessary for dist > 0.001 since inv > 0);
// stage 2 completes the pre-test.
// Lanes with on == false take part in the arithmetic but never in a decision (callers use it for the
// per-lane mesh filter instead of an exec-mask branch around each triangle).
__device__ __forceinline__ void tri_two_stage(const float4& A, const float4& B, const float4& C, const float4& N,
                                              uint32_t i, uint32_t m, f3 o, f3 d, Closest& c, float& best_k,
                                              bool on = true) {
  const f3 n = mk(N.x, N.y, N.z);
  const f3 ao = o - mk(A.x, A.y, A.z);
  TriPre q;
  q.num_t = dot(ao, n);
  const bool front = on & (q.num_t > 0.0f);
  if (!__any(front)) return;
  const float dn = dot(d, n);
  const f3 dao = cross(ao, d);
  q.num_u = dot(mk(C.x, C.y, C.z), dao);
  q.num_v = dot(mk(B.x, B.y, B.z), dao);
  q.det = -dn;
  q.cand = (dn < 0.0f) & front & !pre_reject(q, best_k);
  if (__builtin_expect(__any(q.cand), 0)) {
    if (q.cand) tri_exact(q, i, m, c, best_k);
  }
}

// Triangle sources for the brute-force scan: the std430 buffer (wave-uniform -> SGPRs) or the LDS
// image (3 float4 per triangle = (a.xyz, n.x) (n.yz, e1.xy) (e1.z, e2.xyz)).
struct GlobalTris {
  const float4* __restrict__ t;
  __device__ __forceinline__ void operator()(uint32_t i, float4& A, float4& B, float4& C, float4& N) const {
    A = t[4 * i];
    B = t[4 * i + 1];
    C = t[4 * i + 2];
    N = t[4 * i + 3];
  }
};
struct LdsTris {
  const float4* t;
  __device__ __forceinline__ void operator()(uint32_t i, float4& A, float4& B, float4& C, float4& N) const {
    const float4 p = t[3 * i], q = t[3 * i + 1], r = t[3 * i + 2];
    A = make_float4(p.x, p.y, p.z, 0.0f);
    B = make_float4(q.z, q.w, r.x, 0.0f);
    C = make_float4(r.y, r.z, r.w, 0.0f);
    N = make_float4(p.w, q.x, q.y, 0.0f);
  }
};

// world_hit (raytracing.glsl:267-288) for one lane: spheres, then every triangle of every mesh whose
// (quirky) AABB test passes, two-stage exact test, one running closest hit (ties: first in order).
template <class Src>
__device__ __forceinline__ Closest world_hit_brute(const Scene& sc, const Src& src, const hrt_push_constants& pc, f3 o,
                                                   f3 d, uint32_t& tests) {
  Closest c{kFltMax, 0, 0u, 0u};
  for (int i = 0; i < pc.num_spheres; ++i) {
    const float t = sphere_dist(sc.spheres[i], o, d);
    if (t > 0.001f && t < c.t) c = Closest{t, 1, (uint32_t)i, 0u};
  }
  float best_k = c.t * kOnePlus;  // FLT_MAX*(1+2^-16) = inf: R7 never rejects
  for (int m = 0; m < pc.num_meshes; ++m) {
    const hrt_mesh& mesh = sc.meshes[m];
    const bool pass = aabb_pass(mesh, o, d);
    tests += pass ? mesh.len : 0u;
    if (!pass) continue;
    const uint32_t end = mesh.first_index + mesh.len;
    for (uint32_t i = mesh.first_index; i < end; ++i) {
      float4 A, B, C, N;
      src(i, A, B, C, N);
      tri_two_stage(A, B, C, N, i, (uint32_t)m, o, d, c, best_k);
    }
  }
  return c;
}

// ---- BRUTE / BRUTE_LDS: fused sample/bounce loop ---------------------------------------------------
// Each lane runs its pixel's num_samples paths back to back (RNG state chains through them exactly
// as raytracing.glsl:379-385); the wave iterates until every lane's last path has ended.
template <class Src>
__device__ __forceinline__ void trace_fused(const TraceParams& P, const Src& src, uint32_t x, uint32_t lr) {
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  const hrt_push_constants& pc = P.pc;
  const uint32_t y = global_row(lr, P);
  uint32_t segs = 0, tests = 0;
  const bool active = x < pc.width && lr < P.local_rows && y < pc.height;
  if (active) {
    const uint32_t id = x + y * pc.width;
    f3 colour = mk(0.0f, 0.0f, 0.0f);
    uint32_t state = pc.rng_offset * 719393u + id;
    const float4 rc = sc.rays[id];
    const f3 centre = mk(rc.x, rc.y, rc.z);
    const f3 root = mk(pc.cam_pos[0], pc.cam_pos[1], pc.cam_pos[2]);
    int sample = 0;
    Path p;
    p.bounce = pc.max_bounces + 1;  // "no path in flight"
    while (true) {
      if (p.bounce > pc.max_bounces) {  // start the next sample (or finish)
        if (sample >= pc.num_samples) break;
        ++sample;
        const f3 dir = get_ray_dir(pc, centre, state);
        p = Path{mk(0.0f, 0.0f, 0.0f), mk(1.0f, 1.0f, 1.0f), root, normalize(dir), 0, true};
      }
      const Closest c = world_hit_brute(sc, src, pc, p.pos, p.dir, tests);
      ++segs;
      const bool ended = shade_step(sc, pc, p, c, state);
      ++p.bounce;
      if (ended || p.bounce > pc.max_bounces) {
        colour = colour + p.light * p.colour;
        p.bounce = pc.max_bounces + 1;
      }
    }
    colour = div3(colour, (float)pc.num_samples);
    store_pixel(P, x, lr, colour);
  }
  flush_counters(P, segs, tests);
}

__global__ __launch_bounds__(256) void trace_brute(TraceParams P) {
  uint32_t x, lr;
  lane_pixel(P, x, lr);
  trace_fused(P, GlobalTris{reinterpret_cast<const float4*>(P.tris)}, x, lr);
}

// Whole scene resident in LDS, 1024-thread workgroups (16 waves, a 32x32 pixel tile of 8x8 wave
// tiles): the copy is paid once per workgroup, every wave then streams the triangles from LDS with
// broadcast reads instead of scalar loads.
extern __shared__ float4 lds_tris[];
__global__ __launch_bounds__(1024) void trace_brute_lds(TraceParams P) {
  const uint32_t n = P.n_tris;
  for (uint32_t k = threadIdx.x; k < 3 * n; k += blockDim.x) {
    const uint32_t i = k / 3, part = k - 3 * i;
    const hrt_triangle& t = P.tris[i];
    float4 v;
    if (part == 0) v = make_float4(t.a[0], t.a[1], t.a[2], t.normal[0]);
    else if (part == 1) v = make_float4(t.normal[1], t.normal[2], t.edge_one[0], t.edge_one[1]);
    else v = make_float4(t.edge_one[2], t.edge_two[0], t.edge_two[1], t.edge_two[2]);
    lds_tris[k] = v;
  }
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t x = blockIdx.x * 32 + (wave & 3) * 8 + (lane & 7);
  const uint32_t lr = blockIdx.y * 32 + (wave >> 2) * 8 + (lane >> 3);
  trace_fused(P, LdsTris{lds_tris}, x, lr);
}

// ---- BUNDLE / BUNDLE_CULL ------------------------------------------------------------------------
//
// Per-frame prep (camera_lists): for every mesh, the triangles with num_t = dot(cam_pos - a, n) > 0
// -- computed exactly as a primary lane computes it -- compacted in buffer order into records
// (ao, num_t) (e1, index) (e2, -) (n, -), plus 5 float4 bundle-cull records (g, margin) per triangle.
// A triangle left out cannot be accepted by any primary lane (its dist would be <= 0 or NaN).
//
// Bundle cull: for a primary segment every lane's ray starts at cam_pos, so for a fixed triangle the
// reference's det = -d.n, num_u = d.(e2 x ao) and num_v = d.(e1 x ao) are LINEAR in the lane's
// direction d (ao = cam_pos - a is shared).  Bounding d over the wave's directions (axis a, cosine
// range [c_lo, c_hi], sine bound s_hi) bounds each linear form; a triangle is rejected for the whole
// wave when
//   R1  min d.n            > m_n   (every lane: dn >= 0, raytracing.glsl:217)
//   R3  max d.(e2 x ao)    < -m_u  (every lane: u < 0)
//   R4  min d.(e1 x ao)    > m_v   (every lane: v < 0)
//   R5  min d.(g_u-h+n)    > m_w   (every lane: num_u - num_v > det(1+2^-16), so u, v or w < 0)
// with margins m_* = 1e-5 * (product norms) + 2^-40|n| (+2^-14|n| for R5) covering the rounding of the
// reference's own dot/cross sequence (<= ~10 eps * product norm) and of these bounds.  The cull runs
// lane-parallel: lane j bounds triangle base+j, so 64 triangles cost one pass; survivors (in buffer
// order) get the exact per-lane test.
struct Bundle {
  f3 a;
  float c_lo, c_hi, s_hi;
};

// Wave-uniform cull diagnostics (HRT_OPT_COUNTERS = 2), flushed once per wave.
struct Diag {
  uint32_t prim_iters = 0, prim_considered = 0, prim_survivors = 0;
  uint32_t sec_iters = 0, sec_considered = 0, sec_survivors = 0, sec_lanes = 0;
  uint32_t bvh_visits = 0, bvh_prims = 0, bvh_band = 0;  // per lane (BUNDLE_BVH)
  uint64_t cyc_prim = 0, cyc_sec = 0, cyc_shade = 0;  // shader clocks per wave and phase
  uint32_t sec_stage2 = 0, sec_front = 0;
  uint32_t bvh_trips = 0, bvh_leaf_trips = 0;  // BUNDLE_BVH: wave-level traversal trips
  uint32_t band_max = 0, band_len = 0;          // BUNDLE_WQ: longest band list per batch / every lane's, summed
  uint32_t sky_items = 0;                       // work items run by sky_samples
  uint64_t cyc_sky = 0;                         // ... and their shader clocks
  uint32_t prim_lanes = 0, loop_iters = 0, live_lanes = 0;  // fused-loop lane use
  uint32_t wq_fill[4] = {0, 0, 0, 0};  // BUNDLE_WQ: node steps with 1-16 / 17-32 / 33-48 / 49-64 node pairs
  uint32_t wq_members = 0;             // ... the members of the groups this lane popped (valid slots), summed
  uint32_t dir_lanes = 0;              // lanes whose direction a bounce batch computed (shade_dir)
  uint32_t prim_deferred = 0, batch_only_iters = 0;  // fused loop: trips that ran a batch alone, and their ready lanes
};

__device__ __forceinline__ float wave_min_all(float v) {  // all 64 lanes active
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {  // all 64 lanes active
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Direction cone of the lanes with sel == true (axis = the first such lane's direction).
__device__ __forceinline__ Bundle make_bundle(bool sel, f3 d) {
  const int lead = __builtin_ctzll(__ballot(sel));
  Bundle b;
  b.a = mk(lane_read(d.x, (uint32_t)lead), lane_read(d.y, (uint32_t)lead), lane_read(d.z, (uint32_t)lead));
  const float lam = sel ? dot(d, b.a) : 3.0f;
  b.c_lo = wave_min_all(lam) - 1e-5f;
  b.c_hi = 1.00001f;
  b.s_hi = (b.c_lo > 0.0f) ? __builtin_sqrtf(fmaxf(0.0f, 1.00002f - b.c_lo * b.c_lo)) * 1.00001f + 1e-6f : 1.00001f;
  return b;
}

__device__ __forceinline__ float lin_lower(float ga, float gn, const Bundle& b) {
  return fminf(b.c_lo * ga, b.c_hi * ga) - b.s_hi * gn;
}
__device__ __forceinline__ float lin_upper(float ga, float gn, const Bundle& b) {
  return fmaxf(b.c_lo * ga, b.c_hi * ga) + b.s_hi * gn;
}

// Spheres for the selected lanes (raytracing.glsl:271-276).
__device__ __forceinline__ void spheres_first(const Scene& sc, const hrt_push_constants& pc, bool sel, f3 o, f3 d,
                                              Closest& c) {
  if (!sel) return;
  c = Closest{kFltMax, 0, 0u, 0u};
  for (int i = 0; i < pc.num_spheres; ++i) {
    const float t = sphere_dist(sc.spheres[i], o, d);
    if (t > 0.001f && t < c.t) c = Closest{t, 1, (uint32_t)i, 0u};
  }
}
// ... with the running closest started at `best` (the any-hit traversals of the occlusion queries).
__device__ __forceinline__ void spheres_first(const Scene& sc, const hrt_push_constants& pc, bool sel, f3 o, f3 d,
                                              Closest& c, float best) {
  if (!sel) return;
  c = Closest{best, 0, 0u, 0u};
  for (int i = 0; i < pc.num_spheres; ++i) {
    const float t = sphere_dist(sc.spheres[i], o, d);
    if (t > 0.001f && t < c.t) c = Closest{t, 1, (uint32_t)i, 0u};
  }
}

// Read-only scene data seen through the constant address space: a load with a wave-uniform address
// from it is a scalar (s_load) load.
typedef __attribute__((address_space(4))) const float kfloat;
__device__ __forceinline__ const kfloat* to_const(const float4* p) {
  return (const kfloat*)(const __attribute__((address_space(4))) void*)(p);
}
__device__ __forceinline__ float4 ldk(const kfloat* p, uint32_t i) {  // float4 i of p
  return make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]);
}

// Exact per-lane test of compacted camera-facing record k (ao and num_t precomputed), entered only
// when some lane has dn < 0.
__device__ __forceinline__ void primary_exact_rec(const float4& A, const float4& B, const float4& C, float dn, f3 d,
                                                  uint32_t m, Closest& c, float& best_k) {
  TriPre q;
  q.num_t = A.w;
  const f3 dao = cross(mk(A.x, A.y, A.z), d);
  q.num_u = dot(mk(C.x, C.y, C.z), dao);
  q.num_v = dot(mk(B.x, B.y, B.z), dao);
  q.det = -dn;
  q.cand = (dn < 0.0f) & !pre_reject(q, best_k);
  if (__builtin_expect(__any(q.cand), 0)) {
    if (q.cand) tri_exact(q, __builtin_bit_cast(uint32_t, B.w), m, c, best_k);
  }
}
__device__ __forceinline__ void primary_exact(const kfloat* ct, uint32_t k, float dn, f3 d, uint32_t m, Closest& c,
                                              float& best_k) {
  primary_exact_rec(ldk(ct, 4 * k), ldk(ct, 4 * k + 1), ldk(ct, 4 * k + 2), dn, d, m, c, best_k);
}
// All 64 bytes of camera record k in one scalar load (s_load_dwordx16)
typedef float kf16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(4))) const kf16 kf16c;
__device__ __forceinline__ kf16 ld_rec(const kfloat* ct, uint32_t k) { return *(kf16c*)(ct + 16 * (size_t)k); }

// ---- per-wave primary triangle list ------------------------------------------------------------
// Every primary direction a wave can produce is normalize(M * nc) with nc = centre + (0, t2.y, t1.z),
// |t1.z|, |t2.y| <= jitter_size (get_ray_dir, raytracing.glsl:162-166), i.e. nc in the box X =
// [centre box of the wave's pixels] + [0] x [-j, j] x [-j, j].  The cap around normalize(M * mid(X))
// through the farthest of X's 8 corner directions contains them all (a cap under 90 degrees is
// convex), widened by 1e-5 in cosine for rounding.  The bundle cull against that cap runs ONCE per
// wave; its survivors (camera-list index | mesh << 27, in buffer order) are the only triangles any
// primary segment of the wave can hit, so each primary iteration tests just those.  The list lives
// in one VGPR (entry i in lane i, read back with v_readlane; up to 64 entries) in the LDS-resident
// kernels, and in a per-wave LDS slice of kTileCapLds entries in the others (dense scenes put
// hundreds of triangles in a tile's cap).  A wave whose list overflows culls per iteration.
constexpr uint32_t kTileCapVgpr = 64;
constexpr uint32_t kTileCapLds = 1024;

struct TileList {
  uint32_t v;      // VGPR list: lane i holds entry i
  uint32_t* lds;   // LDS list (nullptr: VGPR list)
  uint32_t n;
  bool ok;
  // aabb_pass of every mesh (<= 8) for a ray from cam_pos by the sign octant of its direction:
  // bit 8m + (sx | sy << 1 | sz << 2) (aabb_truth_table); aabb_ok false -> the literal test
  unsigned long long aabb;
  bool aabb_ok;
  uint32_t tsum;  // lane l: the triangle tests of a primary ray in octant l & 7 (sum of passing meshes' len)
};

// intersecting_aabb's result for origin o depends only on the signs of (bound - o) and of 1/d per
// axis, as long as no product (bound - o) * (1/d) is zero or NaN: each "> 0" test is then a sign
// test, and the quirked min/max chain (raytracing.glsl:199-207) reduces to
//   tx_far > 0 || tx_near > 0 || ty_far > 0 || tz_far > 0 || tz_near > 0.
// So with every bound - o nonzero and not NaN, and |d| <= 1.5 per component (|1/d| >= 2/3, so a
// nonzero product cannot round to 0), aabb_pass(m, o, d) == aabb_pass(m, o, (+-1, +-1, +-1)) with
// d's sign bits (1/+-0 = +-inf keeps the sign).  Lane l evaluates mesh l >> 3 at octant l & 7.
__device__ __forceinline__ void aabb_truth_table(const TraceParams& P, TileList& t) {
  const hrt_push_constants& pc = P.pc;
  const uint32_t lane = threadIdx.x & 63, m = lane >> 3, oct = lane & 7;
  const f3 o = mk(pc.cam_pos[0], pc.cam_pos[1], pc.cam_pos[2]);
  bool pass = false, bad = false;
  uint32_t len = 0;
  if (m < (uint32_t)pc.num_meshes) {
    const hrt_mesh& mesh = kargs()->meshes[m];
    for (int a = 0; a < 3; ++a) {
      const float ov = a == 0 ? o.x : (a == 1 ? o.y : o.z);
      const float lo = mesh.min_point[a] - ov, hi = mesh.max_point[a] - ov;
      bad |= !(lo < 0.0f || lo > 0.0f) || !(hi < 0.0f || hi > 0.0f);  // zero or NaN
    }
    pass = aabb_pass(mesh, o, mk((oct & 1) ? -1.0f : 1.0f, (oct & 2) ? -1.0f : 1.0f, (oct & 4) ? -1.0f : 1.0f));
    len = pass ? mesh.len : 0u;
  }
  t.aabb = __ballot(pass);
  t.aabb_ok = pc.num_meshes <= 8 && !__any(bad);
  // per octant: the tests counter's increment (lanes oct, oct + 8, ... hold its meshes)
  len += (uint32_t)__shfl_xor((int)len, 8, 64);
  len += (uint32_t)__shfl_xor((int)len, 16, 64);
  len += (uint32_t)__shfl_xor((int)len, 32, 64);
  t.tsum = len;
}

// normalize(M * v): a primary direction's arithmetic up to rounding (get_ray_dir forms the same sums with FMAs)
__device__ __forceinline__ f3 box_dir(const hrt_push_constants& pc, f3 v) {
  const float* M = pc.cam_alignment_mat;
  return normalize(mk(M[0] * v.x + M[4] * v.y + M[8] * v.z, M[1] * v.x + M[5] * v.y + M[9] * v.z,
                      M[2] * v.x + M[6] * v.y + M[10] * v.z));
}
__device__ __forceinline__ float jitter_reach(const hrt_push_constants& pc) { return fabsf(pc.jitter_size) * 1.0001f; }

// cdir: lane l < 8 holds the unit direction of corner l of X (bit 0: x, bit 1: y, bit 2: z; hi when set);
// flat: X has no extent in x (lo.x == hi.x), so corners l and l ^ 1 are the same direction.
__device__ __forceinline__ Bundle tile_bundle(const hrt_push_constants& pc, bool active, f3 centre, bool& ok, f3& cdir,
                                              bool& flat) {
  const float inf = __builtin_inff();
  const f3 lo = mk(wave_min_all(active ? centre.x : inf), wave_min_all(active ? centre.y : inf),
                   wave_min_all(active ? centre.z : inf));
  const f3 hi = mk(wave_max_all(active ? centre.x : -inf), wave_max_all(active ? centre.y : -inf),
                   wave_max_all(active ? centre.z : -inf));
  const float j = jitter_reach(pc);
  Bundle b;
  b.a = box_dir(pc, mk(0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y, 0.5f * lo.z + 0.5f * hi.z));
  const uint32_t lane = threadIdx.x & 63;
  const f3 corner = mk((lane & 1) ? hi.x : lo.x, (lane & 2) ? hi.y + j : lo.y - j, (lane & 4) ? hi.z + j : lo.z - j);
  cdir = box_dir(pc, corner);
  flat = lo.x == hi.x;
  const float lam = lane < 8 ? dot(cdir, b.a) : 3.0f;
  b.c_lo = wave_min_all(lam) - 1e-5f;
  b.c_hi = 1.00001f;
  b.s_hi = __builtin_sqrtf(fmaxf(0.0f, 1.00002f - b.c_lo * b.c_lo)) * 1.00001f + 1e-6f;
  // a sane cap (NaN -> false; fminf skips a NaN corner, so a corner that overflowed is checked here)
  ok = b.c_lo > 0.5f && !__any(!(lam == lam));
  return b;
}

// Bundle rules R1, R3-R5 of a cam_cull record (C0..C4) against the cap b.
__device__ __forceinline__ bool bundle_keep(const float4& C0, const float4& C1, const float4& C2, const float4& C3,
                                            const float4& C4, const Bundle& b) {
  const float na = dot(mk(C0.x, C0.y, C0.z), b.a), ua = dot(mk(C1.x, C1.y, C1.z), b.a);
  const float va = dot(mk(C2.x, C2.y, C2.z), b.a), wa = dot(mk(C3.x, C3.y, C3.z), b.a);
  const bool rej = (lin_lower(na, C4.x, b) > C0.w) | (lin_upper(ua, C4.y, b) < -C1.w) |
                   (lin_lower(va, C4.z, b) > C2.w) | (lin_lower(wa, C4.w, b) > C3.w);
  return !rej;
}

// ---- corner rule ---------------------------------------------------------------------------------
// The cap bound is loose twice over: its slope uses |e||ao| where |e x ao| would do (every edge that
// points along the view ray: ground seen at a grazing angle), and each rule has to reject the whole cap
// alone (acute screen-space vertices throw long wedges of false positives).  The same four forms
// evaluated at the CORNER DIRECTIONS of a direction set remove the first cause, and doing so per pixel
// cuts the wedges to pixel size (tools/tile_cull_model.py: island 1080p, 5,639 -> 2,854 tiles with a
// list, 29,086 -> 12,651 entries, no hit tile lost).
//
// Soundness.  A set's primary directions are d = w / |w|, w = M nc, nc in a box B (tile: X above; pixel:
// its own centre + {0} x [-j, j]^2, j = jitter_reach).  B's corners map to w_i = M nc_i with unit
// directions c_i, and nc = sum l_i nc_i with l_i >= 0, sum l_i = 1, so w = sum l_i w_i.  Each form is
// linear in w: if c_i.g < -m for every corner then w.g = sum l_i |w_i| c_i.g < -m sum l_i |w_i| <= -m |w|
// (triangle inequality), i.e. d.g < -m for EVERY direction of the set; likewise c_i.g > m for all i gives
// d.g > m.  So
//   min_i c_i.n > m0,  max_i c_i.gu < -m1,  min_i c_i.h > m2,  min_i c_i.kw > m3
// are R1, R3, R4, R5 with the margins unchanged.  The pixels' boxes cover the item's box, so a triangle
// that every active pixel rejects -- each possibly by another rule -- is rejected for every primary of the
// item by the per-rule argument, rule by rule, pixel by pixel.
// Rounding.  c_i here and the lane's own d are float32 normalize(M nc) (products and sums rounded
// separately here, FMAs in get_ray_dir; nc itself rounded twice): each is within ~6 x 2^-24 of the exact
// unit vector, and a three-term dot product adds 3 x 2^-24 |g|, so a computed c_i.g and the lane's true
// d.g are each off by < 2^-20 |g| ~ 1e-6 |g|.  Every margin is >= 1e-5 x (the product norm >= |g|), of which
// the reference's own dot / cross sequence needs <= ~10 eps ~ 6e-7: the ~9e-6 |g| left cover both.  The
// jitter reach j carries 1e-4 relative; what (c + t1) + t2's rounding can add beyond it (2^-24 |nc|) is a
// direction change of the same 2^-24 order.
// NaN.  A NaN form or margin makes its compare false (keep): the accumulations below start from the first
// corner's value, so a NaN dot product is not skipped by fminf / fmaxf for a finite one; a lane whose own
// corners are not finite keeps everything (the tile's corners are finite when tile_bundle says ok).
struct FormSpan {
  float n, u, h, w;  // min c.n, max c.gu, min c.h, min c.kw over the corners so far
};
__device__ __forceinline__ FormSpan span_at(f3 c, const float4& C0, const float4& C1, const float4& C2,
                                            const float4& C3) {
  return FormSpan{dot(c, mk(C0.x, C0.y, C0.z)), dot(c, mk(C1.x, C1.y, C1.z)), dot(c, mk(C2.x, C2.y, C2.z)),
                  dot(c, mk(C3.x, C3.y, C3.z))};
}
__device__ __forceinline__ FormSpan span_join(const FormSpan& a, const FormSpan& b) {
  return FormSpan{fminf(a.n, b.n), fmaxf(a.u, b.u), fminf(a.h, b.h), fminf(a.w, b.w)};
}
__device__ __forceinline__ bool span_reject(const FormSpan& s, const float4& C0, const float4& C1, const float4& C2,
                                            const float4& C3) {
  return (s.n > C0.w) | (s.u < -C1.w) | (s.h > C2.w) | (s.w > C3.w);
}

// Pixel stage: lane = pixel.  Each active lane holds the 4 corner directions of its own jitter box (one
// pixel's box has no extent in x) and votes on every listed entry; an entry no active lane keeps leaves
// the list, which stays in buffer order.
__device__ __forceinline__ void refine_tile_list(const hrt_push_constants& pc, bool active, f3 centre,
                                                 const float4* cam_cull, TileList& t) {
  const uint32_t lane = threadIdx.x & 63;
  const float j = jitter_reach(pc);
  f3 c[4];
  bool finite = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    c[q] = box_dir(pc, mk(centre.x, (q & 1) ? centre.y + j : centre.y - j, (q & 2) ? centre.z + j : centre.z - j));
    finite &= fabsf(c[q].x) <= 2.0f && fabsf(c[q].y) <= 2.0f && fabsf(c[q].z) <= 2.0f;  // (NaN: false)
  }
  const kfloat* ck = to_const(cam_cull);
  const uint32_t n = __builtin_amdgcn_readfirstlane(t.n);
  uint32_t n2 = 0, v2 = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t e = t.lds ? __builtin_amdgcn_readfirstlane(lds_get(&t.lds[i]))
                             : (uint32_t)__builtin_amdgcn_readlane((int)t.v, (int)i);
    const uint32_t kk = e & 0x07FFFFFFu;
    const float4 C0 = ldk(ck, 5 * kk), C1 = ldk(ck, 5 * kk + 1), C2 = ldk(ck, 5 * kk + 2), C3 = ldk(ck, 5 * kk + 3);
    FormSpan s = span_at(c[0], C0, C1, C2, C3);
#pragma unroll
    for (int q = 1; q < 4; ++q) s = span_join(s, span_at(c[q], C0, C1, C2, C3));
    const bool stay = active && !(finite && span_reject(s, C0, C1, C2, C3));
    if (__any(stay)) {
      if (t.lds) {
        if (lane == 0) lds_put(&t.lds[n2], e);  // n2 <= i: behind the reads (a wave's LDS accesses are in order)
      } else {
        v2 = lane == n2 ? e : v2;
      }
      ++n2;
    }
  }
  t.n = n2;
  if (!t.lds) t.v = v2;
}

// Builds the wave's list (all 64 lanes active; the caller synchronises before reading it): the cap rule,
// then the corner rule on the item's box (tile stage, lane = triangle) and per pixel (refine_tile_list).
// refine false: the cap rule alone (hrt_debug_tile_lists' comparison lists; the trace kernels pass true).
__device__ __forceinline__ TileList build_tile_list(const TraceParams& P, bool active, f3 centre, uint32_t* lds,
                                                    bool refine = true) {
  const hrt_push_constants& pc = P.pc;
  TileList t{0u, lds, 0u, false, 0ull, false, 0u};
  const uint32_t cap = lds ? kTileCapLds : kTileCapVgpr;
  if (pc.num_meshes > 32 || !__any(active)) return t;
  bool ok, flat;
  f3 cdir;
  const Bundle b = tile_bundle(pc, active, centre, ok, cdir, flat);
  if (!ok) return t;
  aabb_truth_table(P, t);
  const uint32_t lane = threadIdx.x & 63;
  const KArgs K = kargs();  // (once per work item)
  const uint32_t* cam_start = K->cam_start;
  const uint32_t* cam_count = K->cam_count;
  const float4* cam_cull = K->cam_cull;
  const uint32_t cstep = __builtin_amdgcn_readfirstlane(flat ? 2u : 1u);  // (every lane holds the same lo, hi)
  for (int m = 0; m < pc.num_meshes; ++m) {
    const uint32_t k0 = cam_start[m], k1 = k0 + cam_count[m];
    for (uint32_t base = k0; base < k1; base += 64) {
      const uint32_t k = base + lane;
      bool keep = false;
      float4 C0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), C1 = C0, C2 = C0, C3 = C0;
      if (k < k1) {
        C0 = cam_cull[5 * k], C1 = cam_cull[5 * k + 1], C2 = cam_cull[5 * k + 2], C3 = cam_cull[5 * k + 3];
        keep = bundle_keep(C0, C1, C2, C3, cam_cull[5 * k + 4], b);
      }
      // tile stage (only passes with a cap survivor: nearly no pass of a sky tile): the item's 8 corner
      // directions, 4 when the box is flat in x, broadcast from the lanes that hold them
      if (refine && __any(keep)) {
        auto corner = [&](uint32_t i) {  // (wave-uniform: v_readlane)
          return mk(bitsf((uint32_t)__builtin_amdgcn_readlane((int)fbits(cdir.x), (int)i)),
                    bitsf((uint32_t)__builtin_amdgcn_readlane((int)fbits(cdir.y), (int)i)),
                    bitsf((uint32_t)__builtin_amdgcn_readlane((int)fbits(cdir.z), (int)i)));
        };
        FormSpan s = span_at(corner(0u), C0, C1, C2, C3);
        for (uint32_t i = cstep; i < 8u; i += cstep) s = span_join(s, span_at(corner(i), C0, C1, C2, C3));
        keep = keep && !span_reject(s, C0, C1, C2, C3);
      }
      unsigned long long mask = __ballot(keep);
      const uint32_t cnt = (uint32_t)__popcll(mask);
      if (t.n + cnt > cap) return t;  // ok stays false: per-iteration cull
      if (lds) {  // lane-parallel append in buffer order
        if (keep) lds_put(&lds[t.n + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))], k | ((uint32_t)m << 27));
        t.n += cnt;
      } else {
        while (mask) {  // few survivors: append each to the next lane
          const uint32_t e = (base + (uint32_t)__builtin_ctzll(mask)) | ((uint32_t)m << 27);
          mask &= mask - 1ull;
          t.v = lane == t.n ? e : t.v;
          ++t.n;
        }
      }
    }
  }
  if (refine && t.n) refine_tile_list(pc, active, centre, cam_cull, t);
  t.ok = true;
  wave_handoff();  // the list's entries (other lanes' stores) before the reads of world_hit_tile
  return t;
}

// Primary segments from the wave's list (ALL 64 lanes active).  Per lane: spheres, the meshes' AABB
// quirk (raytracing.glsl:279) and its test count, then the listed triangles in buffer order.
// Returns the entries it tested (the others: no primary lane's mesh vote; diagnostics).
__device__ __forceinline__ uint32_t world_hit_tile(const Scene& sc, const TraceParams& P, const TileList& tl, bool prim,
                                                   f3 o, f3 d, uint32_t& tests, Closest& c) {
  const hrt_push_constants& pc = P.pc;
  spheres_first(sc, pc, prim, o, d, c);
  // primary lanes start at cam_pos (the table's origin): bit 8m of pm is mesh m's AABB test, by the
  // direction's octant (one 64-bit shift of the wave's table and one lane read of its test count) or,
  // off the table's domain, by the literal test
  const bool octant = tl.aabb_ok && fabsf(d.x) <= 1.5f && fabsf(d.y) <= 1.5f && fabsf(d.z) <= 1.5f;
  const uint32_t oct = (fbits(d.x) >> 31) | ((fbits(d.y) >> 31) << 1) | ((fbits(d.z) >> 31) << 2);
  unsigned long long pm = tl.aabb >> oct;
  const uint32_t oct_tests = lane_read(tl.tsum, oct);
  if (prim && octant) {
    tests += oct_tests;
  } else if (prim) {
    pm = 0ull;
    for (int m = 0; m < pc.num_meshes; ++m) {
      if (aabb_pass(sc.meshes[m], o, d)) {
        pm |= 1ull << (8 * m);
        tests += sc.meshes[m].len;
      }
    }
  }
  float best_k = c.t * kOnePlus;
  const kfloat* ct = to_const(kargs()->cam_tris);
  auto entry = [&](uint32_t i) {
    return tl.lds ? __builtin_amdgcn_readfirstlane(lds_get(&tl.lds[i])) : (uint32_t)__builtin_amdgcn_readlane((int)tl.v, (int)i);
  };
  // (r03: requesting the next entry's record before this one's test was slower, island 2.259 -> 2.338)
  // (the list length through readfirstlane: hipcc had lost its uniformity through build_tile_list's
  // early returns and ran the entry loop as a divergent loop with a VGPR trip count)
  const uint32_t n = __builtin_amdgcn_readfirstlane(tl.n);
  uint32_t tested = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t e = entry(i);
    const uint32_t kk = e & 0x07FFFFFFu, m = e >> 27;
    const bool pass = prim && ((pm >> (8 * m)) & 1ull);
    if (!__any(pass)) continue;
    ++tested;
    {
    // the whole record in one load: the exact test's operands arrive with the normal (one K$ round
    // trip per entry instead of two dependent ones)
    const kf16 R = ld_rec(ct, kk);
    const float dn = pass ? dot(d, mk(R[12], R[13], R[14])) : 0.0f;
    if (__any(dn < 0.0f))
      primary_exact_rec(make_float4(R[0], R[1], R[2], R[3]), make_float4(R[4], R[5], R[6], R[7]),
                        make_float4(R[8], R[9], R[10], R[11]), dn, d, m, c, best_k);
    }
  }
  return tested;
}

// Primary segments of the lanes with prim == true.  Called with ALL 64 lanes of the wave active.
template <bool D>
__device__ __forceinline__ void world_hit_bundle(const Scene& sc, const TraceParams& P, bool prim, f3 o, f3 d,
                                                 uint32_t& tests, Closest& c, Diag& dg) {
  const hrt_push_constants& pc = P.pc;
  const Bundle b = make_bundle(prim, d);
  spheres_first(sc, pc, prim, o, d, c);
  float best_k = c.t * kOnePlus;
  const kfloat* ct = to_const(P.cam_tris);
  const float4* __restrict__ cr = P.cam_cull;
  const uint32_t lane = threadIdx.x & 63;
  for (int m = 0; m < pc.num_meshes; ++m) {
    const hrt_mesh& mesh = sc.meshes[m];
    const bool pass = prim && aabb_pass(mesh, o, d);
    if (prim) tests += pass ? mesh.len : 0u;
    if (!__any(pass)) continue;
    const uint32_t k0 = P.cam_start[m], k1 = k0 + P.cam_count[m];
    for (uint32_t base = k0; base < k1; base += 64) {
      const uint32_t k = base + lane;
      bool keep = false;
      if (k < k1) {
        const float4 C0 = cr[5 * k], C1 = cr[5 * k + 1], C2 = cr[5 * k + 2], C3 = cr[5 * k + 3], C4 = cr[5 * k + 4];
        const float na = dot(mk(C0.x, C0.y, C0.z), b.a), ua = dot(mk(C1.x, C1.y, C1.z), b.a);
        const float va = dot(mk(C2.x, C2.y, C2.z), b.a), wa = dot(mk(C3.x, C3.y, C3.z), b.a);
        const bool rej = (lin_lower(na, C4.x, b) > C0.w) | (lin_upper(ua, C4.y, b) < -C1.w) |
                         (lin_lower(va, C4.z, b) > C2.w) | (lin_lower(wa, C4.w, b) > C3.w);
        keep = !rej;
      }
      unsigned long long mask = __ballot(keep);
      if (D && P.diag) {
        dg.prim_considered += min(64u, k1 - base);
        dg.prim_survivors += (uint32_t)__popcll(mask);
      }
      while (mask) {
        const uint32_t kk = __builtin_amdgcn_readfirstlane(base + (uint32_t)__builtin_ctzll(mask));
        mask &= mask - 1ull;
        if (pass) {
          const float4 N = ldk(ct, 4 * kk + 3);
          const float dn = dot(d, mk(N.x, N.y, N.z));
          if (__any(dn < 0.0f)) primary_exact(ct, kk, dn, d, (uint32_t)m, c, best_k);
        }
      }
    }
  }
}

// Triangle sources of the bounce cull: lane(k) -> (a, n) of triangle k for the lane-parallel cull,
// uniform(k) -> (a, e1, e2, n) of a wave-uniform survivor.
struct CullGlobal {  // std430 buffer; survivors through the constant address space (s_load)
  const float4* __restrict__ T;
  const kfloat* Tk;
  __device__ __forceinline__ void lane(uint32_t k, float4& A, float4& N) const {
    A = T[4 * k];
    N = T[4 * k + 3];
  }
  __device__ __forceinline__ void uniform(uint32_t k, float4& A, float4& B, float4& C, float4& N) const {
    A = ldk(Tk, 4 * k);
    B = ldk(Tk, 4 * k + 1);
    C = ldk(Tk, 4 * k + 2);
    N = ldk(Tk, 4 * k + 3);
  }
};
struct CullLds {  // LDS image, 3 float4 per triangle: (a, n.x) (n.yz, e1.xy) (e1.z, e2)
  const float4* t;
  __device__ __forceinline__ void lane(uint32_t k, float4& A, float4& N) const {
    const float4 p = t[3 * k], q = t[3 * k + 1];
    A = make_float4(p.x, p.y, p.z, 0.0f);
    N = make_float4(p.w, q.x, q.y, 0.0f);
  }
  __device__ __forceinline__ void uniform(uint32_t k, float4& A, float4& B, float4& C, float4& N) const {
    LdsTris{t}(k, A, B, C, N);
  }
};

// ---- cooperative tiles ------------------------------------------------------------------------------
// A heavy tile's frame time is its sequential chain of bounce batches, each a dependent survivor loop
// (profiles/r01k_*).  In a cooperative tile every wave of the workgroup runs the same 64 pixels with
// identical state; the bounce cull's 64-triangle chunks (numbered across meshes in scan order) are
// dealt out over the W waves, chunk j to wave j mod W, and the per-lane closest hits are merged with
// one 64-bit LDS min per lane over
// key = bits(t) << 32 | id, id = 0 for "no triangle" (the sphere / miss result every wave shares)
// and 1 + (mesh << 26 | index) for a triangle.  For t >= 0 the float bits order like t, and the
// reference's scan (spheres, then meshes in order, triangles in index order, strict <) keeps the
// first of equal distances, which is the lowest id: the merge gives exactly the serial result.
// Slots are triple-buffered so that one barrier per batch suffices: wave 0 clears slot r+1 before
// the barrier of batch r, when every wave has finished reading it (batch r-2).
struct Coop {
  uint32_t w, W;                 // this wave, waves in the group (1: not cooperative)
  unsigned long long* ex;        // 3 x 64 slots (LDS)
  uint32_t round;
  uint32_t work;                 // this wave's share of the tile's work units (the planner's cost)
  // persistent loops: the wave sums its items' counters here and flushes them once at the end
  // (three same-address global atomics per item serialised in L2: ~40 ns per item, the floor of
  // low-spp frames -- 4K 4 spp took 5.1 ms per frame)
  bool defer = false;
  unsigned long long acc_s = 0, acc_t = 0, acc_m = 0;
  bool hot = false;              // the item's wave runs at issue priority 3 (tile_loop)
  uint32_t cache_tile = 0xFFFFFFFFu;  // a whole tile's item: its tile (the launch's tile_lists record), else ~0
#if HRT_TIMELINE
  unsigned long long t_setup = 0;  // s_memrealtime when the item's tile list was built (timeline builds)
  unsigned long long t_sky = 0;    // ... 1 if the item ran as a sky item
#endif
};

__device__ __forceinline__ void coop_merge(Coop& co, Closest& c) {
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long* slot = co.ex + 64 * (co.round % 3);
  if (co.w == 0) co.ex[64 * ((co.round + 1) % 3) + lane] = ~0ull;
  const uint32_t id = c.kind == 2 ? ((c.mesh << 26) | c.idx) + 1u : 0u;
  const unsigned long long key = ((unsigned long long)__float_as_uint(c.t) << 32) | id;
  atomicMin(&slot[lane], key);
  __syncthreads();
  const unsigned long long best = slot[lane];
  ++co.round;
  const uint32_t bid = (uint32_t)best;
  if (bid != 0) c = Closest{__uint_as_float((uint32_t)(best >> 32)), 2, (bid - 1u) & 0x03FFFFFFu, (bid - 1u) >> 26};
}

// Bounce segments with a lane-parallel pre-cull (BUNDLE_CULL).  For the bounce lanes (origins o_l,
// directions d_l) and triangle (a, n):
//   S1  num_t = (o - a).n is linear in o: if max over the lanes' origin box B of (o - a).n
//       < -1e-5 |o - a|max |n|_1, every lane computes num_t <= 0 -> dist <= 0 (or NaN): rejected;
//   R1  dn = d.n is linear in d: if min over the lanes' direction cone of d.n > 1e-5 |n|_1, every
//       lane has dn >= 0: rejected.
// Lane j bounds triangle base+j; survivors (buffer order) get the exact per-lane two-stage test.
// Called with ALL 64 lanes active.
template <bool D, class Src>
__device__ __forceinline__ void world_hit_bounce_cull(const Scene& sc, const TraceParams& P, const Src& src, bool sec,
                                                      f3 o, f3 d, uint32_t& tests, Closest& c, Diag& dg, Coop& co) {
  const hrt_push_constants& pc = P.pc;
  const float inf = __builtin_inff();
  const f3 lo = mk(wave_min_all(sec ? o.x : inf), wave_min_all(sec ? o.y : inf), wave_min_all(sec ? o.z : inf));
  const f3 hi = mk(wave_max_all(sec ? o.x : -inf), wave_max_all(sec ? o.y : -inf), wave_max_all(sec ? o.z : -inf));
  const Bundle b = make_bundle(sec, d);
  const bool box_ok = (hi.x - lo.x) <= 3.0e38f && (hi.y - lo.y) <= 3.0e38f && (hi.z - lo.z) <= 3.0e38f;
  const f3 ctr = mk(0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y, 0.5f * lo.z + 0.5f * hi.z);
  // half widths, enlarged so that |o - ctr| <= hw per axis for every bounce lane despite rounding
  const f3 hw = mk((hi.x - ctr.x) * 1.0001f, (hi.y - ctr.y) * 1.0001f, (hi.z - ctr.z) * 1.0001f);
  spheres_first(sc, pc, sec, o, d, c);
  float best_k = c.t * kOnePlus;
  const uint32_t lane = threadIdx.x & 63;
  // cooperative tiles: 64-triangle chunk j of the scan (numbered across meshes) goes to wave j mod W
  const uint32_t cw = __builtin_amdgcn_readfirstlane(co.w);
  uint32_t chunk0 = 0;
  for (int m = 0; m < pc.num_meshes; ++m) {
    const hrt_mesh& mesh = sc.meshes[m];
    const bool pass = sec && aabb_pass(mesh, o, d);
    if (sec) tests += pass ? mesh.len : 0u;
    const uint32_t k0 = mesh.first_index, k1 = k0 + mesh.len;
    const uint32_t skip = (cw + co.W - chunk0 % co.W) % co.W;  // this wave's first chunk of the mesh
    chunk0 += (mesh.len + 63) / 64;
    if (!__any(pass)) continue;
    for (uint32_t base_v = k0 + 64 * skip; base_v < k1; base_v += 64 * co.W) {
      const uint32_t base = __builtin_amdgcn_readfirstlane(base_v);  // uniform: scalar survivor indices
      const uint32_t k = base + lane;
      bool keep = false;
      if (k < k1) {
        float4 A, N;
        src.lane(k, A, N);
        const f3 n = mk(N.x, N.y, N.z);
        const f3 ca = ctr - mk(A.x, A.y, A.z);
        const float an = fabsf(n.x), bn = fabsf(n.y), cn = fabsf(n.z);
        const float nn = an + bn + cn;                                                      // >= |n|
        const float spread = an * hw.x + bn * hw.y + cn * hw.z;                             // max (o - ctr).n
        const float reach = fabsf(ca.x) + fabsf(ca.y) + fabsf(ca.z) + hw.x + hw.y + hw.z;  // >= |o - a|
        const bool s1 = box_ok && (dot(ca, n) + spread + 1e-5f * reach * nn < 0.0f);
        const bool r1 = lin_lower(dot(n, b.a), nn, b) > 1e-5f * nn;
        keep = !(s1 | r1);
      }
      unsigned long long mask = __ballot(keep);
      co.work += 1u + (uint32_t)__popcll(mask);  // one unit per chunk culled and per survivor tested
      if (D && P.diag) {
        dg.sec_considered += min(64u, k1 - base);
        dg.sec_survivors += (uint32_t)__popcll(mask);
      }
      while (mask) {
        // wave-uniform by construction (global source: constant address space -> s_load)
        const uint32_t k1 = __builtin_amdgcn_readfirstlane(base + (uint32_t)__builtin_ctzll(mask));
        mask &= mask - 1ull;
        float4 A, B, C, N;
        src.uniform(k1, A, B, C, N);
        if (D && P.diag && pass) {  // how far the two-stage test gets for this survivor
          const f3 ao = o - mk(A.x, A.y, A.z);
          const bool s2 = dot(ao, mk(N.x, N.y, N.z)) > 0.0f;
          dg.sec_stage2 += __any(s2) ? 1u : 0u;
          dg.sec_front += __any(s2 && dot(d, mk(N.x, N.y, N.z)) < 0.0f) ? 1u : 0u;
        }
        tri_two_stage(A, B, C, N, k1, (uint32_t)m, o, d, c, best_k, pass);
      }
    }
  }
  if (co.W > 1) coop_merge(co, c);
}

// ---- BUNDLE_BVH: per-lane hierarchy traversal for bounce segments ----------------------------------
// Each bounce lane walks the BVH (hrt_bvh.h) in preorder with escape indices (one register of
// state).  For a triangle (a, e1, e2, n) and the lane's ray (o, d), |d| = 1 (DESIGN.md "BVH cull"):
//   back     d.n^ >= 2e-5: the reference's dn = d.n rounds to > 0 and raytracing.glsl:219 rejects;
//   band     -tau_g - 1e-5 < d.n^ < 2e-5 (tau_g = P.bvh_band_tau, the scene's): grazing; the reference's arithmetic is rounding noise
//            there and may accept anywhere in the triangle's plane, so these triangles are listed per
//            cube-map direction cell (hrt_bvh.cpp build_band_lists) and every lane tests its cell's
//            list exactly;
//   front    d.n^ <= -tau with tau >= kBandTau: an accepted triangle's reference (u, v, w) >= 0 puts
//            the exact intersection of the ray's line with the triangle's plane inside the triangle
//            inflated by eta (barycentrics >= -eta), at a line parameter within rel*t + abs of the
//            accepted dist, where
//              eta = 6e + (1.01 rho + 3.2e + 18.4e G R) / (tau - rho - 4e-7)
//              abs = 2.1 (4.2e + rho) R / (tau - rho - 4e-7),  rel = 2.1 (3.2e + rho) / (...) + 4e
//            (e = 2^-24, R >= |o - a| over the node, G and rho from the node record).
// So a node is skipped when its normal cone is entirely back-facing, or when the ray segment
// t in [-abs, best (1 + rel) + abs] misses the node box grown by 2 eta tri_ext (plus coordinate
// rounding) at tau = kBandTau and R = the lane origin's distance to the farthest scene-box corner
// (node margin a + b R and abs = abs_coef R precomputed by hrt_bvh.cpp): no triangle below can then
// be accepted with dist <= best except band triangles, which the band list covers.  Equal distances are
// resolved by the scan key (first in the reference's mesh/index order wins).

// The exact per-lane test of one BVH entry (triangle idx of mesh m, scan key), raytracing.glsl:213-241
// with the running closest (ties: lower key).
__device__ __forceinline__ void bvh_tri_test(const float4& A, const float4& B, const float4& C, const float4& N,
                                             uint32_t key, uint32_t idx, uint32_t m, f3 o, f3 d, Closest& c,
                                             uint32_t& bkey, float& best_k) {
  const f3 n = mk(N.x, N.y, N.z);
  const f3 ao = o - mk(A.x, A.y, A.z);
  TriPre q;
  q.num_t = dot(ao, n);
  if (!(q.num_t > 0.0f)) return;
  const float dn = dot(d, n);
  if (!(dn < 0.0f)) return;
  const f3 dao = cross(ao, d);
  q.num_u = dot(mk(C.x, C.y, C.z), dao);
  q.num_v = dot(mk(B.x, B.y, B.z), dao);
  q.det = -dn;
  if (pre_reject(q, best_k)) return;
  const float inv_det = 1.0f / q.det;
  const float dist = q.num_t * inv_det;
  const float u = q.num_u * inv_det;
  const float v = -q.num_v * inv_det;
  const float w = 1.0f - u - v;
  if (!(dist < 0.0f) && !(u < 0.0f) && !(v < 0.0f) && !(w < 0.0f) && dist > 0.001f &&
      (dist < c.t || (dist == c.t && key < bkey))) {
    c = Closest{dist, 2, idx, m};
    bkey = key;
    best_k = dist * kOnePlus;
  }
}

// BVH entry k from 64 B records (a, key) (e1, mesh) (e2, index) (n, -) (leaf prims, irregular list).
__device__ __forceinline__ void bvh_prim_test(const float4* __restrict__ pr, uint32_t k, unsigned long long mask, f3 o,
                                              f3 d, Closest& c, uint32_t& bkey, float& best_k) {
  const float4 A = pr[4 * k], B = pr[4 * k + 1];
  // all four record loads before the mesh filter (one memory round trip per test, not two: the
  // compiler would otherwise sink C and N below the branch)
  const float4 C = pr[4 * k + 2], N = pr[4 * k + 3];
  asm volatile("; record %0 %1" ::"v"(C.x), "v"(N.x));
  const uint32_t m = __builtin_bit_cast(uint32_t, B.w);
  if (!((mask >> m) & 1ull)) return;  // mesh failed its (quirky) AABB test for this lane
  bvh_tri_test(A, B, C, N, __builtin_bit_cast(uint32_t, A.w), __builtin_bit_cast(uint32_t, C.w), m, o, d, c, bkey,
               best_k);
}

// Hierarchy sources: node k (4 float4) and leaf / band entry k.
struct BvhGlobal {
  const float4* __restrict__ nodes;
  const float4* __restrict__ prims;
  __device__ __forceinline__ void node(uint32_t k, float4& N0, float4& N1, float4& N2, float4& N3) const {
    N0 = nodes[4 * k];
    N1 = nodes[4 * k + 1];
    N2 = nodes[4 * k + 2];
    N3 = nodes[4 * k + 3];
  }
  __device__ __forceinline__ void prim(uint32_t k, unsigned long long mask, f3 o, f3 d, Closest& c, uint32_t& bkey,
                                       float& best_k) const {
    bvh_prim_test(prims, k, mask, o, d, c, bkey, best_k);
  }
};
// The same source for an ANY-HIT traversal (occluded_bvh): world_hit_bounce_bvh then starts the
// running closest at the c.t it is called with (the ray's min(t_max, FLT_MAX)) instead of FLT_MAX, and a lane
// that has accepted anything leaves its loops.  c.kind != 0 is the answer; c is otherwise not a closest hit.
struct BvhGlobalAny : BvhGlobal {};
struct BvhLds {  // nodes and the triangle image in LDS; entry k = triangle | mesh << 26, key = kbase[m] + triangle
  const float4* nodes;
  const float4* tris;
  const uint32_t* entries;
  const uint32_t* kbase;
  __device__ __forceinline__ void node(uint32_t k, float4& N0, float4& N1, float4& N2, float4& N3) const {
    N0 = nodes[4 * k];
    N1 = nodes[4 * k + 1];
    N2 = nodes[4 * k + 2];
    N3 = nodes[4 * k + 3];
  }
  __device__ __forceinline__ void prim(uint32_t k, unsigned long long mask, f3 o, f3 d, Closest& c, uint32_t& bkey,
                                       float& best_k) const {
    const uint32_t e = entries[k], idx = e & 0x03FFFFFFu, m = e >> 26;
    if (!((mask >> m) & 1ull)) return;
    float4 A, B, C, N;
    LdsTris{tris}(idx, A, B, C, N);
    bvh_tri_test(A, B, C, N, kbase[m] + idx, idx, m, o, d, c, bkey, best_k);
  }
};

// true when the node may hold a triangle the reference accepts for (o, d) with dist <= best.
// R >= |o - a| for every vertex of the scene (the lane's origin to the root box's farthest corner),
// abs = abs_coef R: the per-lane part of the node test, computed once per bounce segment.
__device__ __forceinline__ bool bvh_node_visit(const float4& N0, const float4& N1, const float4& N2, const float4& N3,
                                               f3 o, f3 d, f3 inv, float R, float abs_t, float t_hi) {
  const float x = N2.x * d.x + N2.y * d.y + N2.z * d.z;  // cos(angle(d, axis)) within 2e-6
  const float xa = fmaxf(fabsf(x) - 2e-6f, 0.0f);
  const float s_up = __builtin_sqrtf(fmaxf(1.0f - xa * xa, 0.0f)) + 1e-6f;
  if (x * N2.w - s_up * N3.x - 1e-6f > 1e-5f) return false;  // back: every dn > 0
  const float mg = N0.w + N1.w * R;
  const float tx0 = ((N0.x - mg) - o.x) * inv.x, tx1 = ((N1.x + mg) - o.x) * inv.x;
  const float ty0 = ((N0.y - mg) - o.y) * inv.y, ty1 = ((N1.y + mg) - o.y) * inv.y;
  const float tz0 = ((N0.z - mg) - o.z) * inv.z, tz1 = ((N1.z + mg) - o.z) * inv.z;
  const float tn = fmaxf(fmaxf(-abs_t, fminf(tx0, tx1)), fmaxf(fminf(ty0, ty1), fminf(tz0, tz1)));
  const float tf = fminf(fminf(t_hi, fmaxf(tx0, tx1)), fminf(fmaxf(ty0, ty1), fmaxf(tz0, tz1)));
  return !((tn - fabsf(tn) * 1e-6f) > (tf + fabsf(tf) * 1e-6f));  // NaN -> visit
}
// Cube-map cell of a direction (hrt_bvh.cpp face_dir is the inverse): face = 2 * major axis +
// (component < 0), (u, v) = the two minor components over the major one's magnitude.
__device__ __forceinline__ uint32_t dir_cell(f3 d, uint32_t res) {
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  // operands selected per lane, then one pair of divides (the same quotients as dividing inside
  // each face's branch, without a wave running up to three divergent pairs)
  const bool fx = ax >= ay && ax >= az, fy = !fx && ay >= az;
  const uint32_t face = fx ? (d.x < 0.0f ? 1u : 0u) : fy ? (d.y < 0.0f ? 3u : 2u) : (d.z < 0.0f ? 5u : 4u);
  const float den = fx ? ax : fy ? ay : az;
  const float u = (fx ? d.y : fy ? d.z : d.x) / den;
  const float v = (fx ? d.z : fy ? d.x : d.y) / den;
  const float s = 0.5f * (float)res;
  const int iu = min((int)res - 1, max(0, (int)((u + 1.0f) * s)));  // NaN converts to 0
  const int iv = min((int)res - 1, max(0, (int)((v + 1.0f) * s)));
  return (face * res + (uint32_t)iu) * res + (uint32_t)iv;
}

// Grazing-band pre-check: d.n^ of an entry's prim (its unit normal from TraceParams::bvh_band_nhat)
// inside the window (hrt_bvh.h "Grazing-band entries").
struct BandCheck {
  f3 d;
  float lo, hi;
  __device__ __forceinline__ explicit BandCheck(f3 d0, float lo0, float hi0) : d(d0), lo(lo0), hi(hi0) {}
  __device__ __forceinline__ bool in(const float4& nh) const {
    const float dn = __builtin_fmaf(d.z, nh.z, __builtin_fmaf(d.y, nh.y, d.x * nh.x));
    return dn > lo && dn < hi;
  }
};
// Entry k of the band lists: its prim index (16-bit words unless the scene has more than 65536 prims;
// the 16-bit array is padded to whole dwords).  One dword load either way, no branch on the width (a
// branch between a round's loads makes the normal's wait drain the next round's entry load too).
__device__ __forceinline__ uint32_t band_entry(const void* band, uint32_t wide, uint32_t k) {
  const uint32_t w = static_cast<const uint32_t*>(band)[wide ? k : k >> 1];
  return wide ? w : (w >> ((k & 1u) << 4)) & 0xFFFFu;
}

// Bounce segments through the hierarchy.  Called with ALL 64 lanes active (spheres and the
// irregular list are wave-uniform loops; the traversal and the band list are per lane).
template <bool D, class Bvh>
__device__ __forceinline__ void world_hit_bounce_bvh(const Scene& sc, const TraceParams& P, const Bvh& bvh, bool sec,
                                                     f3 o, f3 d, uint32_t& tests, Closest& c, Diag& dg) {
  const hrt_push_constants& pc = P.pc;
  constexpr bool kAny = std::is_same<Bvh, BvhGlobalAny>::value;
  if constexpr (kAny)
    spheres_first(sc, pc, sec, o, d, c, c.t);
  else
    spheres_first(sc, pc, sec, o, d, c);
  unsigned long long mask = 0ull;
  if (sec) {
    for (int m = 0; m < pc.num_meshes; ++m) {
      const hrt_mesh& mesh = sc.meshes[m];
      if (aabb_pass(mesh, o, d)) {
        mask |= 1ull << m;
        tests += mesh.len;
      }
    }
  }
  uint32_t bkey = 0;  // spheres (and "no hit") win every tie
  float best_k = c.t * kOnePlus;
  for (uint32_t k = 0; k < P.bvh_n_irregular; ++k)
    if (sec) bvh_prim_test(P.bvh_irregular, k, mask, o, d, c, bkey, best_k);
  // (any hit: a lane already answered by a sphere or the irregular list skips the band and the nodes; its
  // meshes' lengths are counted above whatever it skips)
  if constexpr (kAny)
    if (c.kind != 0) mask = 0ull;
  const f3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  float R = 0.0f;
  if (P.bvh_n_nodes) {  // farthest root-box corner from the origin, rounded up
    float4 R0, R1, R2, R3;
    bvh.node(0, R0, R1, R2, R3);
    const float fx = fmaxf(fabsf(o.x - R0.x), fabsf(R1.x - o.x)), fy = fmaxf(fabsf(o.y - R0.y), fabsf(R1.y - o.y));
    const float fz = fmaxf(fabsf(o.z - R0.z), fabsf(R1.z - o.z));
    R = __builtin_amdgcn_sqrtf(fx * fx + fy * fy + fz * fz) * 1.0001f;  // 1 ulp, inside the x1.0001
  }
  const float abs_t = P.bvh_abs_coef * R;
  const uint32_t end = P.bvh_n_nodes;
  uint32_t node = (sec && mask) ? 0u : end;
  uint32_t visits = 0, prim_tests = 0, band_tests = 0;
  if (sec && mask) {
    const uint32_t cell = dir_cell(d, P.bvh_dir_res);
    const uint32_t b0 = P.bvh_band_off[cell], b1 = P.bvh_band_off[cell + 1];
    if (D && P.diag) dg.band_len += b1 - b0;  // (the same sum as BUNDLE_WQ's, which reads the cell records)
    // Pre-check: an entry whose d.n^ is outside (-tau_g - 2e-5, 3e-5) is not in this lane's band
    // (-tau_g - 1e-5, 2e-5).
    const BandCheck bc(d, -P.bvh_band_tau - 2e-5f, 3e-5f);
    uint32_t k = b0;
    for (; k + 4 <= b1; k += 4) {
      uint32_t qs[4];
      float4 nh[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) qs[j] = band_entry(P.bvh_band, P.bvh_band_wide, k + j);
#pragma unroll
      for (int j = 0; j < 4; ++j) nh[j] = P.bvh_band_nhat[qs[j]];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (bc.in(nh[j])) {
          bvh.prim(qs[j], mask, o, d, c, bkey, best_k);
          ++band_tests;
        }
      }
      if constexpr (kAny)
        if (c.kind != 0) break;
    }
    for (; k < b1; ++k) {
      if constexpr (kAny)
        if (c.kind != 0) break;
      const uint32_t q = band_entry(P.bvh_band, P.bvh_band_wide, k);
      if (bc.in(P.bvh_band_nhat[q])) {
        bvh.prim(q, mask, o, d, c, bkey, best_k);
        ++band_tests;
      }
    }
    if constexpr (kAny)
      if (c.kind != 0) node = end;
  }
  uint32_t trips = 0, leaf_trips = 0;  // wave-level loop iterations (diagnostics)
  while (node < end) {
    if (D && P.diag) ++trips;
    float4 N0, N1, N2, N3;
    bvh.node(node, N0, N1, N2, N3);
    const uint32_t info = __builtin_bit_cast(uint32_t, N3.z);
    const uint32_t esc = __builtin_bit_cast(uint32_t, N3.w);
    const float t_hi = c.t * (1.0f + P.bvh_rel_t) + abs_t;
    const bool visit = bvh_node_visit(N0, N1, N2, N3, o, d, inv, R, abs_t, t_hi);
    const uint32_t count = info >> 27;
    ++visits;
    if (D && P.diag && __any(visit && count)) ++leaf_trips;
    if (visit && count) {
      const uint32_t first = info & 0x07FFFFFFu;
      for (uint32_t k = first; k < first + count; ++k) bvh.prim(k, mask, o, d, c, bkey, best_k);
      prim_tests += count;
    }
    node = (visit && !count) ? node + 1 : esc;
    if constexpr (kAny)
      if (c.kind != 0) node = end;
  }
  if (D && P.diag) {
    dg.bvh_visits += visits;
    dg.bvh_prims += prim_tests;
    dg.bvh_band += band_tests;
    // trips run by the whole wave: the maximum over its lanes (the loop is divergent)
    dg.bvh_trips += wave_max_u(trips);
    dg.bvh_leaf_trips += wave_max_u(leaf_trips);
  }
}

// ---- BUNDLE_WQ: pair-queue hierarchy traversal for bounce segments --------------------------------
// The per-lane traversal above (BUNDLE_BVH) keeps one node cursor per lane: a wave runs as many
// trips as its longest lane (123 per batch vs 55 visits per lane on island) and a leaf's triangles
// serially, and a heavy 8x8 tile spends ~600K clocks per bounce batch either way (profiles/
// r01k_tile_profiles.jsonl, BUNDLE_CULL_LDS: ~850 survivor triangles x every lane).  Here the work of
// a bounce batch is a set of (ray, node group) and (ray, triangle) PAIRS held in two per-wave LIFO
// stacks in LDS; every step hands 64 pairs of one kind to the 64 lanes, so lanes stay full whatever the
// rays' directions.  A node pair tests every member of a group (the 2..4 children of a kept node of
// the wide image, hrt_bvh.h make_wq_nodes) for its ray, pushes the inner ones (sorted: the farther
// below, and all of a step's nearest children above all its farther ones, so the next step descends
// toward the rays' nearest hits) and the leaves' triangles.  The ray of a pair is read
// from its owner lane (ds_bpermute); its closest hit so far is a 64-bit LDS slot (t bits << 32 |
// (mesh << 26 | triangle) + 1), lowered with ds_min_u64: the minimum over every triangle the
// reference accepts of (dist, scan position), i.e. raytracing.glsl's strict '<' in scan order (spheres
// hold key 0 and win ties, as they are scanned first).  A child is dropped only by BUNDLE_BVH's exact
// node test (wq_node_visit) against the slot's current t, which only ever exceeds the final one.
// When the node stack could overflow, the popped groups' subtrees are walked stacklessly instead.
//
// Settled A/B arms, folded into the code (their switches are gone; the ISA is unchanged by the folding,
// DESIGN.md 15): the nodes' back-face (normal cone) test; the member test without an early-out branch,
// all four slots tested and masked past the group's count (r03s: island -0.6%, cave -0.3%); a member's
// outcome as selects, the cone test squared, the slack compares as fmas (r03t); kept leaves' triangles
// pushed by one loop over the lane's count (r03u: island -1.3%, cave -1.7%); the triangle pre-test's
// rejections as one predicate (r03y: cave -0.4%); pushes by branch, not to a dump word; the band's
// plane-side filter (r03aa: island -0.9%, cave -1.6%); mixed steps; a node step's first member pair read
// before the slot read (r04); band cells read at the band's start, not the batch's (r05b: neutral); band
// rounds one ahead.
#ifndef HRT_WQ_TRI_MIN
#define HRT_WQ_TRI_MIN 64u  // a triangle step runs once this many triangle pairs wait (or no node pair is left)
#endif

// Widest node group the kernel tests per stack entry (hrt_bvh.h kWqMaxWidth).  Measured (r02,
// profiles/r02j_wq_groups_ab.jsonl): 8 slots ran the 4-wide image 9% slower (registers), and the
// triangle stack of an 8-wide image does not fit the LDS; fully ordering the 4 slots (5
// compare-exchanges, HRT_WQ_FULLSORT) instead of only putting the nearest last (3) was 0.9% slower.
// (kWqSlots = 4: hrt_launch_plan.h, whose stack sizing reads it too)

struct WqLds {
  const float4* nodes;        // BVH nodes (LDS copy)
  unsigned long long* slot;   // 64 per wave: closest hit so far per ray (owner lane)
  uint32_t* ns;               // node-group stack: group word (fc | (count - 1) << 16) << 6 | ray
  uint32_t* ts;               // triangle-pair stack: leaf prim << 6 | ray
  uint32_t ncap;              // node stack capacity (>= 256)
  bool capped;                // a kernel under HRT_WQ_VGPR_CAP: slot, ns, ts are wave-uniform (held in SGPRs),
                              // and the wave-uniform values and addresses named at `capped` below stay out of
                              // long-lived VGPRs; the uncapped kernels keep their parent's code
};

__device__ __forceinline__ f3 shfl3(f3 v, uint32_t r) {
  return mk(lane_read(v.x, r), lane_read(v.y, r), lane_read(v.z, r));
}

// BUNDLE_WQ node image (hrt_bvh.h make_wq_nodes): 3 float4 per node, cone in binary16.
__device__ __forceinline__ float half_lo(uint32_t u) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xFFFFu)); }
__device__ __forceinline__ float half_hi(uint32_t u) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16)); }
// The cone's sine from its image word: the image holds S >= sin^2 x 1.00001 (hrt_bvh.h [10]), so
// sqrt(S), widened by the hardware root's error, is an upper bound of sin
__device__ __forceinline__ float wq_sin_up(uint32_t w10) { return __builtin_amdgcn_sqrtf(half_lo(w10)) * 1.0000005f; }
__device__ __forceinline__ uint32_t wq_info(const float4* nodes, uint32_t k) {  // leaf info / right child
  return __builtin_bit_cast(uint32_t, nodes[3 * k + 2].w);
}
__device__ __forceinline__ uint32_t wq_escape(const float4* nodes, uint32_t k) {
  return __builtin_bit_cast(uint32_t, nodes[3 * k + 2].z) >> 16;
}

// The traversal's node source.  BUNDLE_WQ (WqLds): every record in the LDS copy.  BUNDLE_WQ_L2 (WqL2): the
// breadth-first image (hrt_bvh.h make_wq_nodes_bfs), slots below nl -- the top of the tree -- in the LDS
// copy, the others read from global memory (one XCD's L2 holds the whole 3 MB of the largest image).  The
// choice is per node: a group may straddle nl.  The global image is addressed as address space 1, so its
// records are fetched with global_load_dwordx4 / global_load_dword (a generic pointer, or one selected
// between the two sources, would make every node read a flat load; profiles/wq_l2_resources.txt).
typedef float wq_v4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) wq_v4* WqGlobalNodes;
typedef const __attribute__((address_space(1))) uint32_t* WqGlobalWords;
struct WqL2 : WqLds {
  WqGlobalNodes gnodes;  // TraceParams::bvh_wq_nodes_bfs
  uint32_t nl;           // slots kept in LDS (TraceParams::wq_lds_nodes; 0: none)
};
struct WqRec {
  float4 a, b, c;
};
__device__ __forceinline__ float4 wq_f4(wq_v4 v) { return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ WqRec wq_rec(const WqL2& wq, uint32_t k) {
  if (k < wq.nl) {
    const float4* p = wq.nodes + 3 * k;
    return WqRec{p[0], p[1], p[2]};
  }
  const WqGlobalNodes p = wq.gnodes + 3 * k;
  return WqRec{wq_f4(p[0]), wq_f4(p[1]), wq_f4(p[2])};
}
__device__ __forceinline__ uint32_t wq_word(const WqL2& wq, uint32_t k, uint32_t j) {  // word j of slot k's record
  if (k < wq.nl) return __builtin_bit_cast(uint32_t, reinterpret_cast<const float*>(wq.nodes)[12 * k + j]);
  return reinterpret_cast<WqGlobalWords>(wq.gnodes)[12 * k + j];
}
__device__ __forceinline__ uint32_t wq_escape(const WqL2& wq, uint32_t k) { return wq_word(wq, k, 10u) >> 16; }
// compare-exchange of two pushed-child slots: the smaller key (the farther child) first
__device__ __forceinline__ void wq_order(float& ka, uint32_t& ea, float& kb, uint32_t& eb) {
  const bool sw = kb < ka;
  const float k = sw ? kb : ka;
  kb = sw ? ka : kb;
  ka = k;
  const uint32_t e = sw ? eb : ea;
  eb = sw ? ea : eb;
  ea = e;
}

// bvh_node_visit on the 48 B image: the cone axis carries up to kWqAxisErr of binary16 error in d.axis
// (allowed for in both the back-face bound and the sine bound; cos is rounded down and sin up), and
// the hardware square root (1 ulp; +2e-7 keeps the sine an upper bound) -- a node is only ever kept
// more often than by bvh_node_visit.  t_near: the box entry distance (ordering only).
__device__ __forceinline__ bool wq_node_visit_r(const float4& N0, const float4& N1, const float4& N2, f3 o, f3 d,
                                                f3 inv, float R, float abs_t, float t_hi, float& t_near) {
  const uint32_t w8 = __builtin_bit_cast(uint32_t, N2.x), w9 = __builtin_bit_cast(uint32_t, N2.y),
                 w10 = __builtin_bit_cast(uint32_t, N2.z);
  const float x = half_lo(w8) * d.x + half_hi(w8) * d.y + half_lo(w9) * d.z;
  const float xa = fmaxf(fabsf(x) - (2e-6f + kWqAxisErr), 0.0f);
  const float s_up = __builtin_amdgcn_sqrtf(fmaxf(1.0f - xa * xa, 0.0f)) + 1.2e-6f;
  if ((x - kWqAxisErr) * half_hi(w9) - s_up * wq_sin_up(w10) - 1e-6f > 1e-5f) return false;  // back
  const float mg = N0.w + N1.w * R;
  const float tx0 = ((N0.x - mg) - o.x) * inv.x, tx1 = ((N1.x + mg) - o.x) * inv.x;
  const float ty0 = ((N0.y - mg) - o.y) * inv.y, ty1 = ((N1.y + mg) - o.y) * inv.y;
  const float tz0 = ((N0.z - mg) - o.z) * inv.z, tz1 = ((N1.z + mg) - o.z) * inv.z;
  const float tn = fmaxf(fmaxf(-abs_t, fminf(tx0, tx1)), fmaxf(fminf(ty0, ty1), fminf(tz0, tz1)));
  const float tf = fminf(fminf(t_hi, fmaxf(tx0, tx1)), fminf(fmaxf(ty0, ty1), fmaxf(tz0, tz1)));
  t_near = tn;
  return !((tn - fabsf(tn) * 1e-6f) > (tf + fabsf(tf) * 1e-6f));  // NaN -> visit
}
__device__ __forceinline__ bool wq_node_visit(const float4* nd, f3 o, f3 d, f3 inv, float R, float abs_t, float t_hi,
                                              float& t_near) {
  return wq_node_visit_r(nd[0], nd[1], nd[2], o, d, inv, R, abs_t, t_hi, t_near);
}
// A node step's ray, prepared once for the group's members (wq_member_visit).
struct WqRay {
  f3 o, d, inv;
  f3 oi;       // RN(o * inv) per axis
  float sig;   // 2^-23 max |o * inv|: covers the rounding of oi in each slab distance
  float R, abs_t;
};
__device__ __forceinline__ WqRay wq_ray(f3 o, f3 d, f3 inv, float R, float abs_t) {
  WqRay q;
  q.o = o;
  q.d = d;
  q.inv = inv;
  q.R = R;
  q.abs_t = abs_t;
  q.oi = mk(o.x * inv.x, o.y * inv.y, o.z * inv.z);
  q.sig = fmaxf(fmaxf(fabsf(q.oi.x), fabsf(q.oi.y)), fabsf(q.oi.z)) * 0x1p-23f;
  return q;
}
// wq_node_visit_r for a prepared ray, each slab distance as fma(bound, inv, -o inv): the exact
// (bound - o) inv plus at most 2^-24 of the result and 2^-24 |o inv| (the rounding of oi), covered by
// the 1e-6 relative slack and 2 sig on the interval test (one fma instead of a subtract and a
// multiply per bound: island 3.242 -> 3.228 ms, profiles/r02k_node_test_ab.txt).  inv = +-inf gives
// NaN -> visit.  (Measured and dropped: d.axis from binary16 d with v_dot2_f32_f16, 3.345 ms.)
template <bool NodeR>
__device__ __forceinline__ bool wq_member_visit(const float4& N0, const float4& N1, const float4& N2, const WqRay& q,
                                                float t_hi, float& t_near) {
  const uint32_t w8 = __builtin_bit_cast(uint32_t, N2.x), w9 = __builtin_bit_cast(uint32_t, N2.y),
                 w10 = __builtin_bit_cast(uint32_t, N2.z);
  // (fused: each rounding here is far inside the 2e-6 / 1e-6 slacks, and the host's margins carry 1e-6
  // relative headroom over one rounding of a + b R)
  // the first product as an fma with +0 (v_fma_mix_f32 reads the binary16 operand directly)
  const float x = __builtin_fmaf(half_lo(w9), q.d.z, __builtin_fmaf(half_hi(w8), q.d.y, __builtin_fmaf(half_lo(w8), q.d.x, 0.0f)));
  const float xa = fmaxf(fabsf(x) - (2e-6f + kWqAxisErr), 0.0f);
  // (the cone test pays on cave too with per-node radii: without it 7.25 -> 7.43 ms, r03c)
  // The test below squared, without the square root and only ever stricter.  It is back <=> L > s_up sin
  // with L = (x - E) cos - 1.1e-5 and s_up = sqrt(q) + 1.2e-6 (q = max(1 - xa^2, 0); the hardware root is
  // within 1.2e-7 of sqrt(q) on [0, 1]).  Here: L' = (x - E) cos - 1.2e-5 (its two roundings < 2.4e-7
  // below the 1e-6 extra), and s_up^2 <= (sqrt(q) + 1.4e-6)^2 <= q + 3e-6 (sqrt(q) <= 1); the image's
  // S >= sin^2 x 1.00001 (rounded up, hrt_bvh.h [10]) leaves the two roundings of (q2 + 3e-6) S and the one
  // of L'^2 (< 1.8e-7 relative) far inside the x1.00001.  L' > 0 and L'^2 > that imply L > s_up sin.
  // (r04: S precomputed -- one mixed-precision multiply instead of a conversion and three multiplies)
  // NaN -> not back.
  const float q2 = fmaxf(__builtin_fmaf(-xa, xa, 1.0f), 0.0f);
  const float L = __builtin_fmaf(x - kWqAxisErr, half_hi(w9), -1.2e-5f);
  const bool back = L > 0.0f && L * L > __builtin_fmaf(q2 + 3e-6f, half_lo(w10), 0.0f);
  float Rm = q.R;
  if constexpr (NodeR) {  // trace_bundle_wq_nr (HRT_OPT_WQ_NODE_RADIUS)
    // R for this member: the ray origin's distance to the farthest corner of its box (every vertex
    // below lies in the box), x1.0001 over the roundings and the hardware square root
    const float fx = fmaxf(q.o.x - N0.x, N1.x - q.o.x), fy = fmaxf(q.o.y - N0.y, N1.y - q.o.y),
                fz = fmaxf(q.o.z - N0.z, N1.z - q.o.z);
    Rm = fminf(__builtin_amdgcn_sqrtf(__builtin_fmaf(fz, fz, __builtin_fmaf(fy, fy, fx * fx))) * 1.0001f, q.R);
  }
  // (Cone-scaled margins -- c0 + (a + b R) tau_g / tau_e when the member's normal cone bounds -d.n^ >= tau_e
  // > tau_g -- measured slower: cave 6.37 -> 6.60, island 2.25 -> 2.30 ms, profiles/r03/r03g_cone_margin_ab.)
  const float mg = __builtin_fmaf(N1.w, Rm, N0.w);
  const float tx0 = __builtin_fmaf(N0.x - mg, q.inv.x, -q.oi.x), tx1 = __builtin_fmaf(N1.x + mg, q.inv.x, -q.oi.x);
  const float ty0 = __builtin_fmaf(N0.y - mg, q.inv.y, -q.oi.y), ty1 = __builtin_fmaf(N1.y + mg, q.inv.y, -q.oi.y);
  const float tz0 = __builtin_fmaf(N0.z - mg, q.inv.z, -q.oi.z), tz1 = __builtin_fmaf(N1.z + mg, q.inv.z, -q.oi.z);
  const float tn = fmaxf(fmaxf(-q.abs_t, fminf(tx0, tx1)), fmaxf(fminf(ty0, ty1), fminf(tz0, tz1)));
  const float tf = fminf(fminf(t_hi, fmaxf(tx0, tx1)), fminf(fmaxf(ty0, ty1), fmaxf(tz0, tz1)));
  t_near = tn;
  // the 1e-6 relative slacks as fmas (one rounding fewer each; the products' roundings were far inside
  // the slacks either way)
  return !back & !(__builtin_fmaf(-fabsf(tn), 1e-6f, tn) > __builtin_fmaf(fabsf(tf), 1e-6f, tf) + 2.0f * q.sig);
}

// Exact reference test (raytracing.glsl:213-241) of BVH leaf prim record (a, -) (e1, -) (e2, -) (n, -):
// true with dist when the reference accepts the triangle (dist > 0.001, u, v, w >= 0); the division-free
// pre-test (pre_reject) skips candidates beyond best_k first.
__device__ __forceinline__ bool wq_tri_accept(const float4& A, const float4& B, const float4& C, const float4& N, f3 o,
                                              f3 d, float best_k, float& dist) {
  const f3 n = mk(N.x, N.y, N.z);
  const f3 ao = o - mk(A.x, A.y, A.z);
  TriPre q;
  q.num_t = dot(ao, n);
  // the three rejections as one predicate (no early-out branches: in a step of 64 different pairs they
  // almost never skip the whole wave)
  const float dn = dot(d, n);
  const f3 dao = cross(ao, d);
  q.num_u = dot(mk(C.x, C.y, C.z), dao);
  q.num_v = dot(mk(B.x, B.y, B.z), dao);
  q.det = -dn;
  if (!(q.num_t > 0.0f) | !(dn < 0.0f) | pre_reject(q, best_k)) return false;
  const float inv_det = 1.0f / q.det;
  dist = q.num_t * inv_det;
  const float u = q.num_u * inv_det;
  const float v = -q.num_v * inv_det;
  const float w = 1.0f - u - v;
  return !(dist < 0.0f) && !(u < 0.0f) && !(v < 0.0f) && !(w < 0.0f) && dist > 0.001f;
}

// closest-hit slot of ray (lane) r: seeded by its owner, lowered by any lane, read for pruning by any
// lane (a stale value only prunes less: the slot never increases) and finally by its owner
__device__ __forceinline__ void wq_slot_lower(unsigned long long* slot, uint32_t r, unsigned long long v) {
  __hip_atomic_fetch_min(&slot[r], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ float wq_slot_t(const WqLds& wq, uint32_t r) {
  return __uint_as_float(lds_get(reinterpret_cast<const uint32_t*>(wq.slot) + (2 * r + 1)));
}
// The owner's slot.  Capped: its address is formed where it is used, from an opaque copy of the lane index
// (one shift-add on the SGPR base): as an invariant of the item loop it sat in a VGPR, which the capped
// kernels spilled -- a scratch reload and a full vector-memory wait before the seed and before the owner's
// read of every bounce batch.
__device__ __forceinline__ unsigned long long* wq_slot_own(const WqLds& wq, uint32_t lane) {
  if (wq.capped) asm volatile("" : "+v"(lane));
  return &wq.slot[lane];
}
// pair stacks: the lanes with `push` append v in lane order at the wave-uniform top n
__device__ __forceinline__ void wq_push(uint32_t* st, uint32_t& n, bool push, uint32_t v) {
  const unsigned long long b = __ballot(push);
  if (push) lds_put(&st[lanes_below_from(b, n)], v);
  n += (uint32_t)__popcll(b);
}
// One step's pops (world_hit_bounce_wq): lanes [0, nn) read the node stack's entries nc .. nc + nn - 1,
// lanes [nn, nn + tn) the triangle stack's tc .. tc + tn - 1 (nc, tc: the tops after the pops; nn + tn
// <= 64), every other lane gets `idle`.  One load at a selected address and one select: the same words
// as a load per kind under its own branch (three exec splits per step), and a lane of neither kind
// reads the triangle stack's word 0 (always allocated: its capacity is at least 128) and drops it.
__device__ __forceinline__ uint32_t wq_pop(const uint32_t* ns, uint32_t nc, uint32_t nn, const uint32_t* ts,
                                           uint32_t tc, uint32_t tn, uint32_t lane, uint32_t idle) {
  const bool is_node = lane < nn, is_tri = lane - nn < tn;  // (lane - nn wraps past 2^31 for a node lane)
  const uint32_t* p = is_node ? ns + (nc + lane) : ts + (is_tri ? tc + lane - nn : 0u);
  const uint32_t v = lds_get(p);
  return (is_node | is_tri) ? v : idle;
}

// Leaf prim k for ray r (origin o, direction d, mesh filter mask): test and lower the ray's slot.
struct WqTriRec {
  float4 A, B, C, N;
};
__device__ __forceinline__ WqTriRec wq_tri_rec(const float4* __restrict__ pr, uint32_t k) {
  return WqTriRec{pr[4 * k], pr[4 * k + 1], pr[4 * k + 2], pr[4 * k + 3]};
}
__device__ __forceinline__ void wq_tri_test(const WqTriRec& t, const WqLds& wq, uint32_t r, unsigned long long mask,
                                            f3 o, f3 d) {
  const float4 &A = t.A, &B = t.B, &C = t.C, &N = t.N;
  const uint32_t m = __builtin_bit_cast(uint32_t, B.w);
  float dist;
  // the mesh filter (its quirky AABB test for this ray) joins the acceptance instead of leaving
  // first, so the four record loads issue together (one L2 round trip per triangle step, not two)
  if (wq_tri_accept(A, B, C, N, o, d, wq_slot_t(wq, r) * kOnePlus, dist) && ((mask >> m) & 1ull)) {
    const uint32_t id = ((m << 26) | __builtin_bit_cast(uint32_t, C.w)) + 1u;
    wq_slot_lower(wq.slot, r, ((unsigned long long)__float_as_uint(dist) << 32) | id);
  }
}
__device__ __forceinline__ void wq_leaf_prim(const float4* __restrict__ pr, const WqLds& wq, uint32_t k, uint32_t r,
                                             unsigned long long mask, f3 o, f3 d) {
  wq_tri_test(wq_tri_rec(pr, k), wq, r, mask, o, d);
}
// The LDS source for an ANY-HIT pair traversal (occluded_pairs).  world_hit_bounce_wq then seeds
// a ray's slot with the c.t it is called with (the ray's min(t_max, FLT_MAX)) and id 0, and a triangle pair
// that accepts a hit lowers the slot to t = +0 with its (nonzero) id: no genuine t is that low (dist > 0.001),
// so the ray's later node pairs keep no member and its later triangle pairs are dropped -- its remaining
// pairs drain without pushing anything.  id != 0 is the answer; the slot's t is no hit distance.
struct WqLdsAny : WqLds {};
__device__ __forceinline__ void wq_leaf_prim(const float4* __restrict__ pr, const WqLdsAny& wq, uint32_t k, uint32_t r,
                                             unsigned long long mask, f3 o, f3 d) {
  const WqTriRec t = wq_tri_rec(pr, k);
  const uint32_t m = __builtin_bit_cast(uint32_t, t.B.w);
  const float st = wq_slot_t(wq, r);
  float dist;
  if (st > 0.0f && wq_tri_accept(t.A, t.B, t.C, t.N, o, d, st * kOnePlus, dist) && dist < st && ((mask >> m) & 1ull)) {
    const uint32_t id = ((m << 26) | __builtin_bit_cast(uint32_t, t.C.w)) + 1u;
    wq_slot_lower(wq.slot, r, (unsigned long long)id);
  }
}


// The grazing-band lists of a wave's lanes laid end to end (world_hit_bounce_wq): lane l's list of n
// entries starts at global slot pos (exclusive prefix of the lengths), total slots.  slot(base, own)
// gives this lane's slot base + lane of a 64-slot round: its owner lane (the last with pos <= slot and a
// non-empty list) and the owner's entry index (b0 + slot - pos; 0 past the end).  The lanes whose lists
// start in the round mark their start slot (lane + 1, one byte each, in 64 bytes of LDS); a slot's owner
// is the mark at its highest marked slot at or below it, or the previous round's last owner when none is
// (carry).  All 64 lanes active.  hrt_debug_band_flatten runs it on given lists (tests/test_gpu_boundary.py).
struct BandFlat {
  uint8_t* marks;
  uint32_t lane, n, pos, total, delta;  // delta = b0 - pos: entry of slot g = the owner's delta + g (mod 2^32)
  uint32_t carry;
  __device__ __forceinline__ uint32_t slot(uint32_t base, uint32_t& own) {
    // (a slot's mark is another lane's store: with plain accesses hipcc forwarded this lane's own
    // clearing store to the load on the path where the lane marks nothing -- losing the start marks of
    // lists that begin at the slot of a lane with no list of its own; lds_put / lds_get / wave_handoff)
    lds_put(&marks[lane], (uint8_t)0);
    wave_handoff();  // every clear before any lane's mark
    const uint32_t rel = pos - base;
    if (n && rel < 64u) lds_put(&marks[rel], (uint8_t)(lane + 1u));
    wave_handoff();  // every mark before any lane's read
    const uint32_t v = lds_get(&marks[lane]);
    const unsigned long long m = __ballot(v != 0u) & (lane == 63u ? ~0ull : (2ull << lane) - 1ull);
    const uint32_t s = m ? 63u - (uint32_t)__builtin_clzll(m) : 0u;
    const uint32_t sv = lane_read(v, s);
    own = m ? sv - 1u : carry;
    carry = (uint32_t)__builtin_amdgcn_readlane((int)own, 63);
    const uint32_t gi = base + lane;
    owner_delta = lane_read(delta, own);
    const uint32_t k = owner_delta + gi;
    return gi < total ? k : 0u;
  }
  uint32_t owner_delta = 0;  // the last slot()'s owner's delta (its bit 31: the record flag, world_hit_bounce_wq)
};

// A bounce lane's direction cell: its band list's first entry b0 and length n.  With per-cell records
// (TraceParams::bvh_band_rec: 8 dwords per cell -- the list's start, its length, then its first
// kBandInline entries as half-words) one 8-byte load gives both, and a list that fits the record is read
// from it: b0 = the record's first entry as a half-word index of the records, with bit 31 set (the
// slots then load from the line the owner just brought in instead of a second random line).
// Otherwise the offsets (two words of one line) and the list.
constexpr uint32_t kBandInline = 12;
__device__ __forceinline__ void band_cell(const KArgs K, f3 d, uint32_t& b0, uint32_t& n) {
  const uint32_t cell = dir_cell(d, K->bvh_dir_res);
  if (const uint32_t* rec = K->bvh_band_rec) {
    const uint2 h = *reinterpret_cast<const uint2*>(rec + (size_t)cell * 8u);
    n = h.y;
    b0 = n <= kBandInline ? (cell * 16u + 4u) | 0x80000000u : h.x;
  } else {
    const uint32_t* band_off = K->bvh_band_off;
    b0 = band_off[cell];
    n = band_off[cell + 1] - b0;
  }
}

template <bool D, bool NodeR, class Src>
__device__ __forceinline__ void world_hit_bounce_wq(const Scene& sc, const TraceParams& P, const Src& wq, bool sec,
                                                    f3 o, f3 d, uint32_t& tests, Closest& c, Diag& dg) {
  // (every node read below has two arms: the LDS image's statements as they were -- BUNDLE_WQ's kernels are
  // the code they were before the second source -- and the source's accessors)
  constexpr bool kL2 = std::is_same<Src, WqL2>::value;
  const hrt_push_constants& pc = P.pc;
  const uint32_t lane = threadIdx.x & 63;
  // the batch's constants, read here (kargs): live for the batch only
  const KArgs K = kargs();
  const float4* prims = K->bvh_prims;
  const float rel_t = K->bvh_rel_t, abs_coef = K->bvh_abs_coef;
  const uint32_t tcap = K->wq_tcap;
  constexpr bool kAny = std::is_same<Src, WqLdsAny>::value;  // any hit (wq_leaf_prim's overload)
  if constexpr (kAny)
    spheres_first(sc, pc, sec, o, d, c, c.t);
  else
    spheres_first(sc, pc, sec, o, d, c);
  const f3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);  // the meshes' AABB tests and the traversal
  unsigned long long mask = 0ull;
  if (sec) {
    for (int m = 0; m < pc.num_meshes; ++m) {
      const hrt_mesh& mesh = sc.meshes[m];
      if (aabb_pass_inv(mesh, o, inv)) {
        mask |= 1ull << m;
        tests += mesh.len;
      }
    }
  }
  // the irregular list: per lane, as in BUNDLE_BVH
  uint32_t bkey = 0;
  float best_k = c.t * kOnePlus;
  const uint32_t n_irr = K->bvh_n_irregular;
  const float4* irr = K->bvh_irregular;
  for (uint32_t k = 0; k < n_irr; ++k)
    if (sec) bvh_prim_test(irr, k, mask, o, d, c, bkey, best_k);
  // (any hit: a ray already answered by a sphere or the irregular list enters the traversal as an inactive
  // ray -- no band list, no root pair; its meshes' lengths are counted above)
  if constexpr (kAny)
    if (c.kind != 0) mask = 0ull;
  float R;
  {  // farthest root-box corner from the origin, rounded up
    float4 R0, R1;
    if constexpr (kL2) {
      const WqRec rr = wq_rec(wq, 0);
      R0 = rr.a;
      R1 = rr.b;
    } else {
      R0 = wq.nodes[0];
      R1 = wq.nodes[1];
    }
    const float fx = fmaxf(fabsf(o.x - R0.x), fabsf(R1.x - o.x)), fy = fmaxf(fabsf(o.y - R0.y), fabsf(R1.y - o.y));
    const float fz = fmaxf(fabsf(o.z - R0.z), fabsf(R1.z - o.z));
    R = __builtin_amdgcn_sqrtf(fx * fx + fy * fy + fz * fz) * 1.0001f;  // 1 ulp, inside the x1.0001
  }
  const float abs_t = abs_coef * R;
  uint32_t band_tests = 0, band_lmax = 0;
  // the ray's closest hit so far (spheres, the irregular list) seeds its slot
  const uint32_t id0 = c.kind == 2 ? ((c.mesh << 26) | c.idx) + 1u : 0u;
  lds_put(wq_slot_own(wq, lane), ((unsigned long long)__float_as_uint(c.t) << 32) | id0);
  wave_handoff();  // seeds before any lane's read or lowering
  uint32_t tc = 0, tri_pairs = 0, steps = 0;
  // one step of 64 waiting triangle pairs (the band rounds' overflow guard)
  auto tri_step64 = [&]() {
    tc -= 64u;
    wave_handoff();
    const uint32_t e = lds_get(&wq.ts[tc + lane]), r = e & 63u;
    const unsigned long long rm = mask_read(mask, r, K->pc.num_meshes);
    wq_leaf_prim(prims, wq, e >> 6, r, rm, shfl3(o, r), shfl3(d, r));
    wave_handoff();  // these pops before the round's pushes into their words
    tri_pairs += 64u;
    ++steps;
  };
  // Grazing band, flattened over the wave: the bounce lanes' direction-cell lists laid end to end
  // (exclusive prefix pos of their lengths), 64 entries per round whatever the lists' lengths (the
  // per-lane scan ran as long as the batch's longest list: 33 entries against 9.3 per lane on
  // island).  Slot g's list is the last lane with pos <= g; an entry that passes its ray's pre-check
  // becomes a (ray, prim) pair of the triangle steps, whose slot minimum is the per-lane scan's result.
  // r03: the scan is a chain of latencies, not VALU (without it -- wrong frames -- island 2.26 -> 1.99,
  // cave 6.41 -> 5.42 ms): 2-byte entries with the prims' normals in a table (fetched bytes 1.08 ->
  // 0.36 GB per island frame), rounds pipelined one ahead, ballot prefix and start marks instead of
  // 6-step shuffle scans and binary searches: island 2.257 -> 2.154, cave 6.411 -> 6.066 ms
  // (profiles/r03/r03i..r03l; a two-stage pipeline and offsets requested at the bounce's start were
  // no faster).
  if (__any(sec && mask)) {
    const BandCheck bc(d, -K->bvh_band_tau - 2e-5f, 3e-5f);  // see world_hit_bounce_bvh
    // Plane-side filter: an entry whose plane the ray starts behind, s = n^.o - n^.a < -ptol, cannot be
    // accepted.  The reference's num_t = dot(o - a, n) is within 4 eps (|o|_1 + |a|_1) |n| of |n| times
    // the exact n^.(o - a), and s within 6 eps (|o|_1 + |a|_1) of it (n^ within 2^-24 per component, the
    // fma chain, the host's rounding of n^.a, the subtraction), so s < -1e-5 (|o|_1 + max |a|_1) means
    // num_t < 0: dist <= 0, rejected (raytracing.glsl:233-238).  NaN -> kept.
    const float ptol = 1e-5f * (fabsf(o.x) + fabsf(o.y) + fabsf(o.z) + K->bvh_band_a1);
    uint32_t b0 = 0, n = 0;
    if (sec && mask) band_cell(K, d, b0, n);
    if (D && P.diag) {
      dg.band_len += n;
      band_lmax = n;
    }
    // exclusive prefix pos of the lengths and their total (wave_scan_excl; r03 used bit-plane ballots --
    // bvh_band_bits = the bit width of the scene's longest list; a 6-step shuffle scan was slower)
    uint32_t total;
    const uint32_t pos = wave_scan_excl(n, total, K->bvh_band_bits);
    const void* band = K->bvh_band;
    const uint32_t wide = K->bvh_band_wide;
    const float4* nhat = K->bvh_band_nhat;
    // (the node stack's words: empty until the root is tested.  Capped: their address is put in a VGPR for
    // the rounds, by an opaque zero: the rounds otherwise read the uniform base back from a spill lane)
    uint32_t vzero = 0;
    if (wq.capped) asm volatile("" : "+v"(vzero));
    uint8_t* const marks = reinterpret_cast<uint8_t*>(wq.ns) + vzero;
    // (with records, b0 of a list kept in its record is a half-word index of the records with bit 31 set,
    // band_cell: the delta keeps that flag and is taken mod 2^31)
    const uint32_t* rec = K->bvh_band_rec;
    BandFlat bf{marks, lane, n, pos, total, rec ? (b0 & 0x80000000u) | ((b0 - pos) & 0x7FFFFFFFu) : b0 - pos, 0u};
    auto fetch = [&](uint32_t base, uint32_t& own, uint32_t& q) {
      const uint32_t k = bf.slot(base, own);
      if (rec) {  // (kernel argument: wave-uniform) one dword load from the record or the list, no branch
        const uint32_t i = k & 0x7FFFFFFFu;
        const uint32_t* w = (bf.owner_delta >> 31) ? rec : static_cast<const uint32_t*>(band);
        q = (w[i >> 1] >> ((i & 1u) << 4)) & 0xFFFFu;
      } else {
        q = band_entry(band, wide, k);  // (slots past the end: entry 0, unused)
      }
    };
    // Software-pipelined rounds: the next round's owner search and entry load are issued after this
    // round's normal load and before its check, so a round waits for the (cache-resident) normal
    // alone while the next round's (mostly L2-missing) entry load is in flight.  (The last round
    // fetches a round past the end too: a conditional load would make the normal's wait a full drain.)
    uint32_t own = 0, q = 0;
    if (total) fetch(0u, own, q);
    for (uint32_t base = 0; base < total; base += 64u) {
      if (tc + 64u > tcap) tri_step64();  // room for this round's pairs
      const float4 nh = nhat[q];
      uint32_t own_n, q_n;
      fetch(base + 64u, own_n, q_n);
      BandCheck oc = bc;
      oc.d = shfl3(bc.d, own);
      const f3 oo = shfl3(o, own);
      const float ot = lane_read(ptol, own);
      const float sp = __builtin_fmaf(oo.z, nh.z, __builtin_fmaf(oo.y, nh.y, oo.x * nh.x)) - nh.w;
      const bool push = base + lane < total && oc.in(nh) && !(sp < -ot);
      const unsigned long long pb = __ballot(push);
      if (push) lds_put(&wq.ts[lanes_below_from(pb, tc)], (q << 6) | own);
      tc += (uint32_t)__popcll(pb);
      band_tests += push ? 1u : 0u;
      own = own_n;
      q = q_n;
    }
  }
  // pair traversal: the root is tested per lane, then (ray, node group) / (ray, triangle) pairs
  uint32_t rinfo = 0;
  bool rvis = false;
  if (sec && mask) {
    float tn;
    if constexpr (kL2) {
      const WqRec rr = wq_rec(wq, 0);
      rinfo = __builtin_bit_cast(uint32_t, rr.c.w);
      rvis = wq_node_visit_r(rr.a, rr.b, rr.c, o, d, inv, R, abs_t, c.t * (1.0f + rel_t) + abs_t, tn);
    } else {
      rinfo = wq_info(wq.nodes, 0);
      rvis = wq_node_visit(wq.nodes, o, d, inv, R, abs_t, c.t * (1.0f + rel_t) + abs_t, tn);
    }
  }
  const uint32_t rcnt = rvis ? rinfo >> 27 : 0u;
  const unsigned long long rb = __ballot(rvis && rcnt == 0u);
  wave_handoff();  // the band rounds' marks (in the node stack's words) before the root pushes
  if (rvis && rcnt == 0u) lds_put(&wq.ns[lanes_below(rb)], (rinfo << 6) | lane);  // inner root: its children's group
  uint32_t nc = (uint32_t)__popcll(rb);
  if (__any(rcnt != 0u)) {  // leaf root (a scene of at most leaf-size triangles): its triangles, after any band pairs
    uint32_t tot;
    const uint32_t pre = tc + wave_scan_excl(rcnt, tot, 5u);
    for (uint32_t j = 0; j < rcnt; ++j) lds_put(&wq.ts[pre + j], (((rinfo & 0x07FFFFFFu) + j) << 6) | lane);
    tc += tot;
  }
  const uint32_t width = K->bvh_wq_width;  // the image's largest group
  uint32_t node_pairs = 0;
  while (nc | tc) {
    ++steps;
    // Step composition (wave-uniform): triangle pairs when >= 64 wait or no node pair is left; when
    // both stacks are short, one mixed step takes them all (lanes [0, nn) node pairs, then triangles).
    // (Measured, r02: filling a short node step's idle lanes with triangle pairs, or running triangle
    // steps from 32 waiting pairs, was no faster: 3.699 / 3.722 vs 3.692 ms, profiles/r02g_ab.txt.)
    const bool tri_step = tc >= HRT_WQ_TRI_MIN || nc == 0u;
    const bool mixed = !tri_step && tc > 0u && nc + tc <= 64u;
    const uint32_t tn = tri_step ? min(64u, tc) : (mixed ? tc : 0u);
    const uint32_t nn = tri_step ? 0u : min(64u, nc);
    tc -= tn;
    nc -= nn;
    node_pairs += nn;
    tri_pairs += tn;
    const bool overflow = nc + width * nn > wq.ncap;  // wave-uniform
    const bool is_node = lane < nn, is_tri = lane - nn < tn;  // (lane - nn wraps past 2^31 for a node lane)
    if (D && P.diag && nn) ++dg.wq_fill[(nn - 1u) >> 4];
    wave_handoff();  // the last step's pushes and slot lowerings before this step's pops and reads
    const uint32_t e = wq_pop(wq.ns, nc, nn, wq.ts, tc, tn, lane, lane);
    const uint32_t r = e & 63u;
    const f3 ro = shfl3(o, r), rd = shfl3(d, r);
    const unsigned long long rm = mask_read(mask, r, K->pc.num_meshes);
    if (is_tri) wq_leaf_prim(prims, wq, e >> 6, r, rm, ro, rd);
    if (nn == 0u) continue;
    // node pairs (ray r, group fc .. fc + cnt - 1): test every member.  Slot k: member k's push entry
    // (its info word << 6 | r when a kept inner node, else ~0u), sort key (minus its box entry
    // distance when pushed, else -inf), and its triangle count when a kept leaf.
    // (r03, measured slower: fetching the mesh filter only for steps with triangle pairs and abs_t as
    // abs_coef * R instead of a shuffle -- island 2.271 -> 2.276, cave 7.248 -> 7.310 ms)
    const f3 rinv = shfl3(inv, r);
    const float rR = lane_read(R, r), rabs = lane_read(abs_t, r);
    const WqRay rq = wq_ray(ro, rd, rinv, rR, rabs);
    uint32_t pe[kWqSlots], li[kWqSlots];
    float pk[kWqSlots];
#pragma unroll
    for (int k = 0; k < (int)kWqSlots; ++k) {
      pe[k] = ~0u;
      li[k] = 0u;
      pk[k] = -kFltMax;
    }
    if (is_node) {
      const uint32_t g = e >> 6, fc = g & 0xFFFFu, gcnt = (g >> 16) + 1u;
      if (D && P.diag) dg.wq_members += gcnt;
      if (!overflow) {
        // the first member pair's records are requested before the slot read: that read is an atomic
        // (lds_get), which the scheduler keeps every other memory access on its side of, so requested
        // after it they waited for the ray shuffles and the slot before being issued
        float4 A00, A01, A02, B00, B01, B02;
        if constexpr (kL2) {
          const WqRec ra0 = wq_rec(wq, fc), rb0 = wq_rec(wq, fc + min(1u, gcnt - 1u));
          A00 = ra0.a, A01 = ra0.b, A02 = ra0.c, B00 = rb0.a, B01 = rb0.b, B02 = rb0.c;
        } else {
          const float4* na0 = wq.nodes + 3 * fc;
          const float4* nb0 = wq.nodes + 3 * (fc + min(1u, gcnt - 1u));
          A00 = na0[0], A01 = na0[1], A02 = na0[2], B00 = nb0[0], B01 = nb0[1], B02 = nb0[2];
        }
        // (both pairs up front: 24 more live VGPRs, scratch 92 -> 160 B with spills in the fused loop)
        float t_any = 1.0f;  // any hit: the slot's t, +0 once the ray is answered (then no member is kept)
        if constexpr (kAny) t_any = wq_slot_t(wq, r);
        const float t_hi = (kAny ? t_any : wq_slot_t(wq, r)) * (1.0f + rel_t) + rabs;
        auto member = [&](const float4& N0, const float4& N1, const float4& N2, int k, bool valid = true) {
          float tnear;
          const uint32_t inf = __builtin_bit_cast(uint32_t, N2.w);
          // the outcome as selects: no branch, and the info word arrives with the record (a branch let
          // hipcc sink its LDS read into the kept path: one more dependent round trip per member)
          const bool vis = wq_member_visit<NodeR>(N0, N1, N2, rq, t_hi, tnear) & valid & (!kAny || t_any > 0.0f);
          const bool leaf = (inf >> 27) != 0u;
          li[k] = (vis & leaf) ? inf : 0u;
          pe[k] = (vis & !leaf) ? ((inf << 6) | r) : ~0u;
          pk[k] = (vis & !leaf) ? -tnear : -kFltMax;
        };
        // members two at a time, both records read up front (six LDS reads in flight); every group
        // has >= 2 members, and an odd count reads its last member twice and keeps one
        // every slot is tested, the ones past the group's count masked (no per-pair branch)
#pragma unroll
        for (int h = 0; h < (int)kWqSlots / 2; ++h) {
          if (h == 0) {
            member(A00, A01, A02, 0);
            member(B00, B01, B02, 1);
            continue;
          }
          float4 A0, A1, A2, B0, B1, B2;
          if constexpr (kL2) {
            const WqRec ra = wq_rec(wq, fc + min(2u * h, gcnt - 1u)), rb = wq_rec(wq, fc + min(2u * h + 1u, gcnt - 1u));
            A0 = ra.a, A1 = ra.b, A2 = ra.c, B0 = rb.a, B1 = rb.b, B2 = rb.c;
          } else {
            const float4* na = wq.nodes + 3 * (fc + min(2u * h, gcnt - 1u));
            const float4* nb = wq.nodes + 3 * (fc + min(2u * h + 1u, gcnt - 1u));
            A0 = na[0], A1 = na[1], A2 = na[2], B0 = nb[0], B1 = nb[1], B2 = nb[2];
          }
          member(A0, A1, A2, 2 * h, h == 0 || 2u * h < gcnt);
          member(B0, B1, B2, 2 * h + 1, h == 0 || 2u * h + 1u < gcnt);
        }
        // the nearest member in the last slot (pushed last = popped first)
#pragma unroll
        for (int st = 1; st < (int)kWqSlots; st *= 2)
#pragma unroll
          for (int k = st - 1; k + st < (int)kWqSlots; k += 2 * st) wq_order(pk[k], pe[k], pk[k + st], pe[k + st]);
      } else {  // finish the group's subtrees with a stackless walk (escape links)
        uint32_t end;
        if constexpr (kL2)
          end = wq_escape(wq, fc + gcnt - 1u);
        else
          end = wq_escape(wq.nodes, fc + gcnt - 1u);
        uint32_t cur = fc;
        while (cur != end) {
          uint32_t inf;
          WqRec rc;
          if constexpr (kL2) {
            rc = wq_rec(wq, cur);
            inf = __builtin_bit_cast(uint32_t, rc.c.w);
          } else {
            inf = wq_info(wq.nodes, cur);
          }
          const uint32_t cnt = inf >> 27;
          float tnear;
          const float t_hi = wq_slot_t(wq, r) * (1.0f + rel_t) + rabs;
          bool v;
          if constexpr (kL2)
            v = wq_node_visit_r(rc.a, rc.b, rc.c, ro, rd, rinv, rR, rabs, t_hi, tnear);
          else
            v = wq_node_visit(wq.nodes + 3 * cur, ro, rd, rinv, rR, rabs, t_hi, tnear);
          if (v && cnt) {
            const uint32_t first = inf & 0x07FFFFFFu;
            for (uint32_t k = first; k < first + cnt; ++k) wq_leaf_prim(prims, wq, k, r, rm, ro, rd);
          }
          if constexpr (kL2)  // (the escape from the record just read)
            cur = (v && !cnt) ? (inf & 0xFFFFu) : __builtin_bit_cast(uint32_t, rc.c.z) >> 16;
          else
            cur = (v && !cnt) ? (inf & 0xFFFFu) : wq_escape(wq.nodes, cur);  // inner: its first child
        }
      }
    }
    // kept inner members: slot-major (every lane's slot 0, then slot 1, ...; the ordering may have
    // moved a member to any slot)
    wave_handoff();  // this step's pops before the pushes that reuse their words
#pragma unroll
    for (int k = 0; k < (int)kWqSlots; ++k) {
      const bool push = pe[k] != ~0u;
      const unsigned long long bk = __ballot(push);
      if (push) lds_put(&wq.ns[lanes_below_from(bk, nc)], pe[k]);
      nc += (uint32_t)__popcll(bk);
    }
    // kept leaves' triangles: exclusive prefix of the per-lane counts (0..16)
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < (int)kWqSlots; ++k) cnt += li[k] >> 27;
    // (a step that kept no leaf -- the upper levels of every batch -- skips the scan and the pushes: the
    // scan of all-zero counts gives tot = 0 and no lane has an entry, so the stacks are left the same)
    if (!__any(cnt != 0u)) continue;
    uint32_t tot;
    const uint32_t pre = wave_scan_excl(cnt, tot, 5u);
    if (tc + tot <= tcap) {  // wave-uniform
      uint32_t at = tc + pre;
      // one loop over the lane's kept triangles (slot of entry j by its running start, selects),
      // instead of a loop per slot
      const uint32_t c0 = li[0] >> 27, c1 = li[1] >> 27, c2 = li[2] >> 27;
      const uint32_t s1 = c0, s2 = s1 + c1, s3 = s2 + c2;
      const uint32_t f0 = li[0] & 0x07FFFFFFu, f1 = (li[1] & 0x07FFFFFFu) - s1, f2 = (li[2] & 0x07FFFFFFu) - s2,
                     f3 = (li[3] & 0x07FFFFFFu) - s3;
      // (the slot picked by a two-level select -- s1 <= s2 <= s3: j >= s2 leaves f2 / f3 by s3, j < s2
      // leaves f0 / f1 by s1 -- whose two inner selects do not wait for each other)
      for (uint32_t j = 0; j < cnt; ++j) {
        const uint32_t f = j >= s2 ? (j >= s3 ? f3 : f2) : (j >= s1 ? f1 : f0);
        lds_put(&wq.ts[at + j], ((f + j) << 6) | r);
      }
      tc += tot;
    } else {  // a burst of kept leaves beyond the triangle stack: each lane tests its own in place
#pragma unroll
      for (int k = 0; k < (int)kWqSlots; ++k) {
        const uint32_t c = li[k] >> 27, first = li[k] & 0x07FFFFFFu;
        for (uint32_t j = 0; j < c; ++j) wq_leaf_prim(prims, wq, first + j, r, rm, ro, rd);
      }
    }
  }
  wave_handoff();  // every lowering before the owners' reads
  if (sec) {
    const unsigned long long s = lds_get(wq_slot_own(wq, lane));
    const uint32_t id = (uint32_t)s;
    if (id != 0u) c = Closest{__uint_as_float((uint32_t)(s >> 32)), 2, (id - 1u) & 0x03FFFFFFu, (id - 1u) >> 26};
  }
  if (D && P.diag) {  // wave totals, held by lane 0 (the tile record sums lanes)
    if (lane == 0) {
      dg.bvh_visits += node_pairs;
      dg.bvh_prims += tri_pairs;
      dg.bvh_trips += steps;
    }
    dg.bvh_band += band_tests;
    const uint32_t bm = wave_max_u(band_lmax);
    if (lane == 0) dg.band_max += bm;
  }
}

// Fused loop of BUNDLE / BUNDLE_CULL / BUNDLE_BVH.  Every lane stays in the loop until the whole wave is done, so
// the loop top is a full-wave region (lane-parallel culls and shuffles need all 64 lanes).  Primary
// segments take the bundle path; a lane whose next segment is a bounce waits (state untouched) until
// at least sec_batch lanes wait or no primary segment is left in the wave, then all waiting lanes run
// their bounce segment together.  Per-pixel order of work (and so every result) is unchanged.

// Sky items.  A wave whose primary list is empty (tl.ok, tl.n == 0) in a scene without spheres tests
// nothing in world_hit_tile, so each primary segment of its lanes is a miss: raytracing.glsl:318-346's
// miss branch (environment light, path ends, no RNG draw after get_ray_dir) and the lane's next sample
// starts at once.  The fused loop then spends its whole trip on bookkeeping (ballots, the bounce-batch
// vote, the list loop's set-up, shade_step's branches) around one ray generation.  sky_samples runs the
// lanes' num_samples such segments as a plain loop instead, two samples per trip (once each sample's
// three hashes are drawn, their ray generations are independent), with the fused loop's per-pixel
// arithmetic in the same order: the same colour, RNG state, segment and test counts.
#ifndef HRT_SKY_LOOP
#define HRT_SKY_LOOP 1
#endif
#ifndef HRT_SKY_UNROLL
#define HRT_SKY_UNROLL 1  // samples per trip of the sky loop (r04i/j: 1 beats 2 by ~1% on island; 3, 4 no better)
#endif
template <bool Zero>
__device__ __forceinline__ void sky_segment(const KArgs K, const TileList& tl, bool active, f3 centre, uint32_t& state,
                                            f3& colour, uint32_t& tests) {
  const auto& pc = K->pc;
  const f3 dir = get_ray_dir_sky<Zero>(pc, centre, state);
  // unit: the wave's second normalize took its fast path, so |d.c| <= 1 + 2^-23 in every lane (normalize_wu)
  bool unit = false;
  const f3 d = HRT_NORM_UNIFORM ? normalize_wu(dir, unit) : normalize(dir);
  // world_hit_tile's test count: the octant table (one lane read, all 64 lanes run this), or the
  // literal AABB test off its domain (|d.c| <= 1.5: implied by unit)
  // (the octant's byte address for ds_bpermute directly: __shfl added the lane's 64-lane segment base)
  const uint32_t oct4 = ((fbits(d.x) >> 31) << 2) | ((fbits(d.y) >> 31) << 3) | ((fbits(d.z) >> 31) << 4);
  const uint32_t oct_tests = (uint32_t)__builtin_amdgcn_ds_bpermute((int)oct4, (int)tl.tsum);
  if (__builtin_expect(tl.aabb_ok && (unit || (fabsf(d.x) <= 1.5f && fabsf(d.y) <= 1.5f && fabsf(d.z) <= 1.5f)), 1)) {
    tests += oct_tests;
  } else if (active) {
    const f3 o = mk(pc.cam_pos[0], pc.cam_pos[1], pc.cam_pos[2]);
    for (int m = 0; m < pc.num_meshes; ++m)
      if (aabb_pass(K->meshes[m], o, d)) tests += K->meshes[m].len;
  }
  // shade_step's miss (p.light = 0 + environment light) and the caller's colour += light * (1, 1, 1).
  // With |d.y| <= 1 + 2^-23 each light component is (1 - a) + a k with a = (d.y + 1) / 2 in
  // [-2^-24, 1 + 2^-24] and k in [0.5, 1]: at least 0.5 - 2^-23, never a zero, so 0 + light == light
  // (and without the environment light it is +0 either way).
  f3 light = environment_light(pc, d);
  if (!unit) light = mk(0.0f, 0.0f, 0.0f) + light;
  colour = colour + light * mk(1.0f, 1.0f, 1.0f);
}
// The lanes' whole pixels.  ALL 64 lanes run it (wave-uniform condition; the idle lanes' results are
// dropped); tl holds the wave's octant table.
__device__ __forceinline__ void sky_samples(const TileList& tl, bool active, f3 centre, uint32_t& state, f3& colour,
                                            uint32_t& segs, uint32_t& tests) {
  const KArgs K = kargs();
  const int ns = K->pc.num_samples;
  uint32_t t = 0;
  int s = 0;
  if (HRT_SKY_ZERO && fabsf(K->pc.jitter_size) < __builtin_inff() &&
      __all(!active || (centre.x != 0.0f && centre.y != 0.0f && fabsf(centre.x) < __builtin_inff() &&
                        fabsf(centre.y) < __builtin_inff()))) {  // get_ray_dir_sky<true>'s premises
    for (; s + HRT_SKY_UNROLL <= ns; s += HRT_SKY_UNROLL) {
#pragma unroll
      for (int u = 0; u < HRT_SKY_UNROLL; ++u) sky_segment<true>(K, tl, active, centre, state, colour, t);
    }
    for (; s < ns; ++s) sky_segment<true>(K, tl, active, centre, state, colour, t);
  } else {
    for (; s + HRT_SKY_UNROLL <= ns; s += HRT_SKY_UNROLL) {
#pragma unroll
      for (int u = 0; u < HRT_SKY_UNROLL; ++u) sky_segment<false>(K, tl, active, centre, state, colour, t);
    }
    for (; s < ns; ++s) sky_segment<false>(K, tl, active, centre, state, colour, t);
  }
  if (active) {
    segs += ns > 0 ? (uint32_t)ns : 0u;
    tests += t;
  }
}

// Issue priorities (s_setprio): heavy items' waves run at 3 (tile_loop), a light item's wave at 0 and
// at HRT_BOUNCE_PRIO during its bounce traversals -- the dependent LDS / L2 chains go first and the
// other waves' ALU work fills in behind them (r04z: cave 5.508 -> 5.433 ms per frame, island unchanged;
// light items at 1 or 2 with sky waves at 0, or bounce priority 2 or 3, no better;
// profiles/r04/r04z*_ab_*.jsonl)
#ifndef HRT_BOUNCE_PRIO
#define HRT_BOUNCE_PRIO 1
#endif
// kBounceWqR: BUNDLE_WQ with node margins from each member's own R (HRT_OPT_WQ_NODE_RADIUS = 2)
// kBounceWqL2 / kBounceWqL2R: the same two with the node source of BUNDLE_WQ_L2 (WqL2)
enum BounceMode {
  kBounceBrute = 0,
  kBounceCull = 1,
  kBounceBvh = 2,
  kBounceWq = 3,
  kBounceWqR = 4,
  kBounceWqL2 = 5,
  kBounceWqL2R = 6
};
constexpr bool is_wq(int b) { return b == kBounceWq || b == kBounceWqR || b == kBounceWqL2 || b == kBounceWqL2R; }
constexpr bool is_wq_node_r(int b) { return b == kBounceWqR || b == kBounceWqL2R; }

#ifndef HRT_PIXEL_POOL
#define HRT_PIXEL_POOL 1
#endif
template <int Bounce, bool D, class CullSrc, class BvhSrc = BvhGlobal>
__device__ __forceinline__ void trace_fused_split(const TraceParams& P, uint32_t x, uint32_t lr, const CullSrc& csrc,
                                                  const BvhSrc& bsrc, uint32_t* list_lds, Coop& co,
                                                  uint32_t frame = 0, uint32_t nrun = 1) {
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  const hrt_push_constants& pc = P.pc;
  const GlobalTris src{reinterpret_cast<const float4*>(P.tris)};
  uint32_t y = global_row(lr, P);
  uint32_t segs = 0, tests = 0;
  const bool active = x < pc.width && lr < kargs()->local_rows && y < pc.height;
  uint32_t id = active ? x + y * pc.width : 0u;
  const uint64_t tile_t0 = (D && P.tile_cycles) ? __builtin_readcyclecounter() : 0;
  f3 colour = mk(0.0f, 0.0f, 0.0f);
  uint32_t state = (pc.rng_offset + frame) * 719393u + id;  // raytracing.glsl:376, frame f of the launch
  f3 centre = mk(0.0f, 0.0f, 0.0f);
  if (active) {
    const float4 rc = kargs()->rays[id];
    centre = mk(rc.x, rc.y, rc.z);
  }
#if HRT_TL_PREPASS
  // a whole tile's item: the list the launch's tile_lists kernel built for the tile (the same function of
  // the same inputs -- camera, the tile's ray centres, the camera lists -- as building it here, which the
  // launch's other frames of the tile would repeat; r05c timelines: ~11 us of dependent L2 round trips
  // per item, 6 wave-us per tile-frame on island, 13 on a rank of 8)
  TileList tl;
  if (co.cache_tile != 0xFFFFFFFFu && !list_lds) {
    const uint32_t* rec = kargs()->tl_cache + (size_t)co.cache_tile * kTlRecWords;
    const uint32_t lane = threadIdx.x & 63;
    tl.v = rec[lane];
    tl.tsum = rec[64 + lane];
    tl.lds = nullptr;
    tl.n = __builtin_amdgcn_readfirstlane(rec[128]);
    tl.ok = __builtin_amdgcn_readfirstlane(rec[129]) != 0u;
    tl.aabb = (unsigned long long)__builtin_amdgcn_readfirstlane(rec[130]) |
              ((unsigned long long)__builtin_amdgcn_readfirstlane(rec[131]) << 32);
    tl.aabb_ok = __builtin_amdgcn_readfirstlane(rec[132]) != 0u;
  } else {
    tl = build_tile_list(P, active, centre, list_lds);
  }
  // (both arms give wave-uniform n and aabb, but hipcc merges them per lane: three VGPRs held for the whole
  // item, which the capped kernels spilled and reloaded from scratch on every primary trip)
  if constexpr (is_wq(Bounce)) {
    if (bsrc.capped) {
      tl.n = __builtin_amdgcn_readfirstlane(tl.n);
      tl.aabb = (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)tl.aabb) |
                ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(tl.aabb >> 32)) << 32);
    }
  }
#else
  const TileList tl = build_tile_list(P, active, centre, list_lds);
#endif
#if HRT_TIMELINE
  co.t_setup = __builtin_amdgcn_s_memrealtime();
  co.t_sky = tl.ok && tl.n == 0u && pc.num_spheres == 0;
#endif
  // bounce batch threshold scaled to the item's active lanes (a split tile's row group has 8/k rows):
  // a batch of few lanes then runs alongside the other lanes' primary segments instead of after them
  const uint32_t nactive = (uint32_t)__popcll(__ballot(active));
  const uint32_t sec_thresh = max(1u, (kargs()->sec_batch * nactive + 63u) / 64u);
  // ... and the primary phase's threshold beside a batch, scaled the same way
  const uint32_t prim_thresh = max(1u, (kargs()->prim_batch * nactive + 63u) / 64u);
  int sample = 0;
  Path p;
  p.bounce = pc.max_bounces + 1;
  // the direction a surviving hit still owes (shade_hit / shade_dir).  Set only in a lane that then waits
  // (0 < p.bounce <= max_bounces) and cleared by the batch every waiting lane joins, so it ends before
  // the lane's next sample, pixel-frame or frame; an item's idle lanes never shade.
  Pending<is_wq(Bounce)> pd;
  bool done = !active;
  Diag dg;
  // Frame runs (tile_loop): the item's frames frame .. frame + nrun - 1 of a multi-frame launch, one
  // after the other per lane -- a lane that finishes its pixel in one frame starts the pixel's next
  // frame (rng_offset + f, its own image) at once instead of idling until the wave's slowest lane ends.
  uint32_t fr = 0;
  // Pixel pool (HRT_PIXEL_POOL, a whole tile's frame run with every lane active): the run's 64 x nrun
  // pixel-frames are one pool, frame-major, and a lane that finishes a pixel-frame takes the pool's next
  // one -- any pixel of the tile, not only its own pixel's next frame -- so the wave ends one pixel-frame
  // after the pool empties instead of after its slowest pixel's nrun frames.  A pixel-frame's work is
  // the same whichever lane runs it (its RNG seed, centre, samples in order, its own image), so every
  // frame is unchanged.  A lane that takes another pixel reloads its ray centre (a line the item's
  // start brought into the cache); fr = nrun once the pool is empty and the lane's last pixel-frame is
  // stored.
  const bool pool = HRT_PIXEL_POOL && nrun > 1u && __all(active);
  uint32_t pool_next = 64u;  // (wave-uniform)
  if (HRT_SKY_LOOP && tl.ok && tl.n == 0u && pc.num_spheres == 0) {  // wave-uniform: every segment a miss
    const uint64_t s0 = (D && P.diag) ? __builtin_readcyclecounter() : 0;
    for (;; ++fr) {
      sky_samples(tl, active, centre, state, colour, segs, tests);
      if (fr + 1u >= nrun) break;
      if (active) store_pixel(P, x, lr, div3(colour, (float)pc.num_samples), frame + fr);
      colour = mk(0.0f, 0.0f, 0.0f);
      state = (pc.rng_offset + frame + fr + 1u) * 719393u + id;
    }
    const uint32_t ns = pc.num_samples > 0 ? (uint32_t)pc.num_samples : 0u;
    if (co.w == 0) co.work += (2u + 3u * ns) * nrun;  // the fused loop's work units for these trips
    if (D && P.diag) {
      dg.prim_iters += ns * nrun;
      dg.sky_items += nrun;
      dg.cyc_sky += __builtin_readcyclecounter() - s0;
    }
    done = true;
  }
  while (__any(!done)) {
    // (a loop: with num_samples <= 0 a new pixel-frame ends at once too, and each must still be stored)
    while (pool) {
      const bool need = !done && p.bounce > pc.max_bounces && sample >= pc.num_samples;
      const unsigned long long nb = __ballot(need);
      if (!nb) break;
      {
        if (need) store_pixel(P, x, lr, div3(colour, (float)pc.num_samples), frame + fr);
        const uint32_t idx = pool_next + lanes_below(nb);
        pool_next += (uint32_t)__popcll(nb);
        if (need) {
          if (idx < 64u * nrun) {
            const uint32_t px = idx & 63u;
            fr = idx >> 6;
            x = (x & ~7u) + (px & 7u);
            lr = (lr & ~7u) + (px >> 3);
            y = global_row(lr, P);
            id = x + y * pc.width;
            const float4 rc = kargs()->rays[id];
            centre = mk(rc.x, rc.y, rc.z);
            colour = mk(0.0f, 0.0f, 0.0f);
            sample = 0;
            state = (pc.rng_offset + frame + fr) * 719393u + id;
          } else {
            done = true;
            fr = nrun;
          }
        }
      }
    }
    // ready: the lane's path has ended and its pixel-frame has a sample left, which starts in the trip
    // that runs its primary segment (below).  A lane with no sample left (and, pooled, no pool entry: the
    // refill above made it done) is done here, whatever the trip runs, and never counts as ready.
    bool ready = false;
    if (!done && p.bounce > pc.max_bounces) {
      // (a while: with num_samples <= 0 every frame of the run ends at once and each must still be stored)
      while (!pool && sample >= pc.num_samples && fr + 1u < nrun) {  // the pixel's next frame of the run
        store_pixel(P, x, lr, div3(colour, (float)pc.num_samples), frame + fr);
        ++fr;
        colour = mk(0.0f, 0.0f, 0.0f);
        sample = 0;
        state = (pc.rng_offset + frame + fr) * 719393u + id;
      }
      if (sample >= pc.num_samples) {
        done = true;
      } else {
        ready = true;
      }
    }
    const bool waiting = !done && !ready;  // 0 < p.bounce <= max_bounces: a bounce segment to run
    const uint32_t nwait = (uint32_t)__popcll(__ballot(waiting));
    const uint32_t nready = (uint32_t)__popcll(__ballot(ready));
    // The phases run when their lanes are full: the batch once sec_thresh lanes wait, or
    // when no lane is ready; the primary phase in a trip without a batch, and beside a batch once
    // prim_thresh lanes are ready (1: in every trip with a ready lane).  A deferred lane keeps its state
    // and draws nothing, exactly as a waiting lane does, so its pixel's samples and RNG draws keep their order.
    // (r04d, measured and dropped: primary segments waiting too while a bounce batch runs and fewer than
    // 8 lanes have one -- island 1.859 -> 1.878 ms)
    // Progress: a lane that is not done is ready or waiting.  nready > 0 without a batch runs the primary
    // phase, nready == 0 leaves nwait > 0 and runs the batch: every trip with a live lane runs a phase,
    // and a phase runs one of the finitely many segments of each lane in it.
    const bool run_sec = nwait > 0 && (nwait >= sec_thresh || nready == 0);
    const bool run_prim = nready > 0 && (!run_sec || nready >= prim_thresh);
    const bool prim = ready && run_prim;
    const bool sec = waiting && run_sec;
    if (prim) {
      ++sample;
      // the camera (matrix, jitter, position) read at the sample's start (kargs): 13 values not held
      // in SGPRs across the loop
      const KArgs K = kargs();
      const f3 dir = get_ray_dir(K->pc, centre, state);
      p = Path{mk(0.0f, 0.0f, 0.0f), mk(1.0f, 1.0f, 1.0f), mk(K->pc.cam_pos[0], K->pc.cam_pos[1], K->pc.cam_pos[2]),
               normalize_fl(dir), 0, true};
    }
    Closest c{kFltMax, 0, 0u, 0u};
    uint64_t t0 = 0, t1 = 0, t2 = 0, tb = 0;
    if (D && P.diag) {
      dg.prim_iters += run_prim ? 1u : 0u;
      dg.sec_iters += run_sec ? 1u : 0u;
      dg.sec_lanes += run_sec ? nwait : 0u;
      dg.prim_lanes += run_prim ? nready : 0u;
      dg.prim_deferred += run_prim ? 0u : nready;  // (then a batch runs: nready > 0 without one runs the phase)
      dg.batch_only_iters += run_sec && !run_prim ? 1u : 0u;
      // (an item's last trip only finds every lane done and runs nothing: not counted, so that every
      // counted trip ran a phase)
      dg.loop_iters += nready + nwait > 0 ? 1u : 0u;
      dg.live_lanes += (uint32_t)__popcll(__ballot(!done));
      t0 = __builtin_readcyclecounter();
    }
    if (co.w == 0) co.work += 2u + (run_prim ? 1u + (tl.ok ? tl.n : 64u) : 0u);  // shading, primary list
    if (run_prim) {
      if (tl.ok) {
        const uint32_t tested = world_hit_tile(kscene(), P, tl, prim, p.pos, p.dir, tests, c);
        if (D && P.diag) {
          dg.prim_considered += tl.n;
          dg.prim_survivors += tested;
        }
      } else {
        world_hit_bundle<D>(sc, P, prim, p.pos, p.dir, tests, c, dg);
      }
    }
    if (D && P.diag) t1 = __builtin_readcyclecounter();
    if (run_sec) {
      const bool owed = sec && pd.id != 0u;
      if (D && P.diag) dg.dir_lanes += (uint32_t)__popcll(__ballot(owed));
      if (owed) shade_dir(kscene(), p, state, pd);
      if (D && P.diag) tb = __builtin_readcyclecounter() - t1;  // (shading's clocks)
      if (HRT_BOUNCE_PRIO && !co.hot) __builtin_amdgcn_s_setprio(HRT_BOUNCE_PRIO);
      if constexpr (is_wq(Bounce)) {
        world_hit_bounce_wq<D, is_wq_node_r(Bounce)>(kscene(), P, bsrc, sec, p.pos, p.dir, tests,
                                                     c, dg);
      } else if constexpr (Bounce == kBounceBvh) {
        world_hit_bounce_bvh<D>(sc, P, bsrc, sec, p.pos, p.dir, tests, c, dg);
      } else if constexpr (Bounce == kBounceCull) {
        world_hit_bounce_cull<D>(sc, P, csrc, sec, p.pos, p.dir, tests, c, dg, co);
      } else {
        if (sec) c = world_hit_brute(sc, src, pc, p.pos, p.dir, tests);
      }
    }
    if (HRT_BOUNCE_PRIO && run_sec && !co.hot) __builtin_amdgcn_s_setprio(0);
    if (D && P.diag) t2 = __builtin_readcyclecounter();
    if (prim || sec) {
      ++segs;
      const bool ended = shade_hit(kscene(), pc, p, c, state, p.bounce >= pc.max_bounces, pd);
      ++p.bounce;
      if (ended || p.bounce > pc.max_bounces) {
        colour = colour + p.light * p.colour;
        p.bounce = pc.max_bounces + 1;
      }
    }
    if (D && P.diag) {
      const uint64_t t3 = __builtin_readcyclecounter();
      dg.cyc_prim += t1 - t0;
      dg.cyc_sec += t2 - t1 - tb;
      dg.cyc_shade += t3 - t2 + tb;
    }
  }
  if (co.w != 0) return;  // cooperative tile: wave 0 of the group writes the results
  if (active && fr < nrun) {
    colour = div3(colour, (float)pc.num_samples);
    store_pixel(P, x, lr, colour, frame + fr);
  }
  if (co.defer) {
    unsigned long long s, t;
    uint32_t mx;
    wave_counters(segs, tests, s, t, mx);
    co.acc_s += s;
    co.acc_t += t;
    co.acc_m += mx;
  } else {
    flush_counters(P, segs, tests);
  }
  if (D && P.tile_cycles && (threadIdx.x & 63) == 0) {  // lane 0 sits at the tile's (0, 0)
    const uint32_t tiles_x = (pc.width + 7) / 8;
    unsigned long long* rec = P.tile_cycles + 4 * ((lr / 8) * tiles_x + x / 8);
    atomicMax(&rec[0], (unsigned long long)(__builtin_readcyclecounter() - tile_t0));  // slowest item of a split tile
    // bounce batches | (BUNDLE_WQ) pair steps << 32
    atomicAdd(&rec[1], (unsigned long long)dg.sec_iters |
                           (is_wq(Bounce) ? (unsigned long long)dg.bvh_trips << 32 : 0ull));
    if (Bounce != kBounceBvh && !is_wq(Bounce)) atomicAdd(&rec[2], (unsigned long long)dg.sec_survivors);
    atomicAdd(&rec[3], (unsigned long long)dg.cyc_sec);
  }
  if (D && P.tile_cycles && (Bounce == kBounceBvh || is_wq(Bounce)) && active) {
    // BUNDLE_BVH: the tile's per-lane node visits, summed | (leaf + band triangle tests) << 32
    const uint32_t tiles_x = (pc.width + 7) / 8;
    atomicAdd(P.tile_cycles + 4 * ((lr / 8) * tiles_x + x / 8) + 2,
              (unsigned long long)dg.bvh_visits + ((unsigned long long)(dg.bvh_prims + dg.bvh_band) << 32));
  }
  if (D && P.diag && (threadIdx.x & 63) == 0) {
    atomicAdd(&P.diag[10], (unsigned long long)dg.cyc_prim);
    atomicAdd(&P.diag[11], (unsigned long long)dg.cyc_sec);
    atomicAdd(&P.diag[12], (unsigned long long)dg.cyc_shade);
    atomicAdd(&P.diag[13], (unsigned long long)dg.sec_stage2);
    atomicAdd(&P.diag[14], (unsigned long long)dg.sec_front);
    atomicAdd(&P.diag[15], (unsigned long long)dg.bvh_trips);
    atomicAdd(&P.diag[16], (unsigned long long)dg.bvh_leaf_trips);
    atomicAdd(&P.diag[17], (unsigned long long)dg.band_max);
    atomicAdd(&P.diag[0], (unsigned long long)dg.prim_iters);
    atomicAdd(&P.diag[1], (unsigned long long)dg.prim_considered);
    atomicAdd(&P.diag[2], (unsigned long long)dg.prim_survivors);
    atomicAdd(&P.diag[3], (unsigned long long)dg.sec_iters);
    atomicAdd(&P.diag[4], (unsigned long long)dg.sec_considered);
    atomicAdd(&P.diag[5], (unsigned long long)dg.sec_survivors);
    atomicAdd(&P.diag[6], (unsigned long long)dg.sec_lanes);
    if (dg.sky_items) {
      atomicAdd(&P.diag[19], (unsigned long long)dg.sky_items);
      atomicAdd(&P.diag[20], (unsigned long long)dg.cyc_sky);
    }
    atomicAdd(&P.diag[21], (unsigned long long)dg.prim_lanes);
    atomicAdd(&P.diag[22], (unsigned long long)dg.loop_iters);
    atomicAdd(&P.diag[23], (unsigned long long)dg.live_lanes);
    if (dg.batch_only_iters) {
      atomicAdd(&P.diag[30], (unsigned long long)dg.prim_deferred);
      atomicAdd(&P.diag[31], (unsigned long long)dg.batch_only_iters);
    }
    if (is_wq(Bounce)) {
#pragma unroll
      for (int b = 0; b < 4; ++b) atomicAdd(&P.diag[24 + b], (unsigned long long)dg.wq_fill[b]);
    }
  }
  if (D && P.diag && is_wq(Bounce) && dg.wq_members) atomicAdd(&P.diag[28], (unsigned long long)dg.wq_members);
  if (D && P.diag && dg.dir_lanes && (threadIdx.x & 63) == 0) atomicAdd(&P.diag[29], (unsigned long long)dg.dir_lanes);
  if (D && P.diag && (Bounce == kBounceBvh || is_wq(Bounce))) {
    atomicAdd(&P.diag[7], (unsigned long long)dg.bvh_visits);
    atomicAdd(&P.diag[8], (unsigned long long)dg.bvh_prims);
    atomicAdd(&P.diag[9], (unsigned long long)dg.bvh_band);
    atomicAdd(&P.diag[18], (unsigned long long)dg.band_len);
  }
}

template <bool D>
__global__ __launch_bounds__(256) void trace_bundle(TraceParams P) {
  __shared__ uint32_t lists[4 * kTileCapLds];
  uint32_t x, lr;
  lane_pixel(P, x, lr);
  const float4* T = reinterpret_cast<const float4*>(P.tris);
  Coop solo{0u, 1u, nullptr, 0u, 0u};
  trace_fused_split<kBounceBrute, D>(P, x, lr, CullGlobal{T, to_const(T)}, BvhGlobal{},
                                     lists + (threadIdx.x >> 6) * kTileCapLds, solo);
}

#ifndef HRT_CULL_WAVES
#define HRT_CULL_WAVES 1
#endif
template <bool D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HRT_CULL_WAVES))) void trace_bundle_cull(
    TraceParams P) {
  __shared__ uint32_t lists[4 * kTileCapLds];
  uint32_t x, lr;
  lane_pixel(P, x, lr);
  const float4* T = reinterpret_cast<const float4*>(P.tris);
  Coop solo{0u, 1u, nullptr, 0u, 0u};
  trace_fused_split<kBounceCull, D>(P, x, lr, CullGlobal{T, to_const(T)}, BvhGlobal{},
                                    lists + (threadIdx.x >> 6) * kTileCapLds, solo);
}

template <bool D>
__global__ __launch_bounds__(256) void trace_bundle_bvh(TraceParams P) {
  __shared__ uint32_t lists[4 * kTileCapLds];
  uint32_t x, lr;
  lane_pixel(P, x, lr);
  const float4* T = reinterpret_cast<const float4*>(P.tris);
  Coop solo{0u, 1u, nullptr, 0u, 0u};
  trace_fused_split<kBounceBvh, D>(P, x, lr, CullGlobal{T, to_const(T)}, BvhGlobal{P.bvh_nodes, P.bvh_prims},
                                   lists + (threadIdx.x >> 6) * kTileCapLds, solo);
}


// Stage the triangle buffer into LDS in the BRUTE_LDS image (3 float4 per triangle).
__device__ __forceinline__ void stage_tris(const TraceParams& P, float4* dst, uint32_t block) {
  const uint32_t n = P.n_tris;
  for (uint32_t k = threadIdx.x; k < 3 * n; k += block) {
    const uint32_t i = k / 3, part = k - 3 * i;
    const hrt_triangle& t = P.tris[i];
    float4 v;
    if (part == 0) v = make_float4(t.a[0], t.a[1], t.a[2], t.normal[0]);
    else if (part == 1) v = make_float4(t.normal[1], t.normal[2], t.edge_one[0], t.edge_one[1]);
    else v = make_float4(t.edge_one[2], t.edge_two[0], t.edge_two[1], t.edge_two[2]);
    dst[k] = v;
  }
}

// Persistent tile loop of the LDS-resident variants: the workgroups stay resident (one or two per CU,
// the scene staged once) and each wave takes 8x8 pixel tiles from a global counter until the image
// is done, so no wave idles while a slower wave of its workgroup finishes.  Every wave leaves the
// loop once the counter passes the tile count.
//
// Work items (P.items, built by plan_fill from the previous trace's per-tile costs): tile | log2 K << 22
// | s << 25 | heavy << 31.  K == 1 is a whole tile; otherwise item s (0..K-1) covers the tile's pixels
// [s * 64/K, (s+1) * 64/K) in row-major order with 64/K lanes (the rest idle); K (2..64) grows with
// the tile's cost.  A heavy tile's pixels run as K shorter sample chains in parallel
// with lighter batches, and the planner puts them first.  Every pixel is computed exactly once and
// independently of which wave runs it, so the bytes do not depend on the plan.  Each item's cost goes
// to P.tile_cost[tile] for the next plan: deterministic work units (Coop::work: survivor tests,
// culled chunks, primary list entries, iterations; the same with or without cooperation) in
// BUNDLE_CULL_LDS, shader clocks / 16 in BUNDLE_BVH_LDS.
// The work queue: one u64 word, the front cursor (tile_loop) in its low half and the back cursor
// (trace_sky) in its high half, both in work units (item x frame) -- the back cursor counted down from
// the plan's end n; sched[kSchedSky] = the number of sky items the plan ends in (plan_scan; 0 without a
// sky lane), S = that x nf units.  Crossing rule: every claim is one atomic add on the word, so the claims
// are totally ordered and each returns both cursors as they stood.
//  - A front claim of g that returns (f, b) owns the units [f, f + g) below n - min(b, S): the units
//    from there up belong to back claims made already.
//  - A back claim of r that returns (f, b) with b < S owns [max(n - min(b + r, S), f), n - b): the units
//    under f went to earlier front claims, whose bound was at least n - b (they saw at most b units
//    claimed), and every later front claim sees at least b + r and stops at n - min(b + r, S) or below.
//    With b >= S, or f >= n - b (the cursors have crossed: every lower unit is under f too), it owns
//    nothing and the wave ends.  Back claims past S only raise a count that front claims clamp to S, so
//    trace_sky never takes a unit below the sky items.
// So every unit has exactly one owner whichever side arrives first, and either side finishes the other's end.
// (kItemTileMask, kSchedSky, kSchedQueue and the planner's helpers: hrt_plan.h)
// Sky: the kernel may run beside trace_sky and makes front claims as above; otherwise nothing ever raises
// the word's high half and the loop counts on its low half alone.
template <int BLOCK, bool CoopOk, bool Sky = false, class Body>
__device__ __forceinline__ void tile_loop(const TraceParams& P, unsigned long long* ex, uint32_t* s_item, Body&& body) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t tiles_x = (P.pc.width + 7) / 8, tiles = tiles_x * ((P.local_rows + 7) / 8);
  // A launch of nf frames runs every item once per frame: work index t is item t / nf of frame t % nf,
  // so each item's frames follow each other and the plan's longest-first order holds across frames.
  const uint32_t nf = P.n_frames > 1 ? P.n_frames : 1u;
  const uint32_t n = (P.items ? P.sched[1] : tiles) * nf;
  uint32_t first = 0;
  // Phase 1 (a plan with cooperative heavy tiles): the workgroup takes the heavy items [0, H) one
  // at a time, all its waves on the same tile (Coop).  The item index goes through LDS; at the loop
  // head each wave's lane 0 publishes its share of the previous tile's work units.
  if (CoopOk && P.items && P.coop) {
    const uint32_t H = P.sched[2] * nf;
    first = H;
    Coop co{threadIdx.x >> 6, (uint32_t)BLOCK / 64, ex, 0u, 0u};
    uint32_t prev_tile = 0xFFFFFFFFu, prev_cost = 0;
    for (;;) {
      if (lane == 0) {
        if (prev_tile != 0xFFFFFFFFu) {
          atomicAdd(&P.tile_cost[prev_tile], prev_cost);
          atomicAdd(reinterpret_cast<unsigned long long*>(P.sched + 6), (unsigned long long)prev_cost);
        }
        if (threadIdx.x == 0) *s_item = atomicAdd(&P.sched[5], 1u);
      }
      __syncthreads();
      const uint32_t h = __builtin_amdgcn_readfirstlane(*s_item);
      __syncthreads();
      if (h >= H) break;
      const uint32_t hi = h / nf, hf = h - hi * nf;
      const uint32_t tile = __builtin_amdgcn_readfirstlane(P.items[hi]) & kItemTileMask;
      const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
      co.work = 0;
      body(tx * 8 + (lane & 7), ty * 8 + (lane >> 3), co, hf, 1u);
      prev_cost = __builtin_amdgcn_readfirstlane(co.work);
      prev_tile = tile;
    }
    if (lane == 0 && prev_tile != 0xFFFFFFFFu) {
      atomicAdd(&P.tile_cost[prev_tile], prev_cost);
      atomicAdd(reinterpret_cast<unsigned long long*>(P.sched + 6), (unsigned long long)prev_cost);
    }
  }
  // Phase 2: every wave on its own.  The loop's only lane-divergent block is at its head (lane 0
  // publishes the previous item's cost and takes the next item).  A second lane-0 block at the latch
  // let the compiler thread lanes 1-63 straight back to the body past the head, where they spun on
  // a stale item: keep it this way.
  Coop solo{0u, 1u, nullptr, 0u, 0u};
  solo.defer = true;
  uint32_t prev_tile = 0xFFFFFFFFu, prev_cost = 0, prev_lk = 0;
  // Items are taken kGrab at a time while far from the end (one same-address atomic per kGrab items;
  // the plan's longest-first order is kept, and the last HRT_GRAB_TAIL items per resident wave go singly).
  // The threshold sum of the planner (sched[6]) is summed per wave and added once.
#ifndef HRT_GRAB
#define HRT_GRAB 4u
#endif
#ifndef HRT_FRAME_RUN
#define HRT_FRAME_RUN 1
#endif
  constexpr uint32_t kGrab = HRT_GRAB;
#ifndef HRT_GRAB_TAIL
#define HRT_GRAB_TAIL 64u  // items per resident wave taken singly at the end (16 x the r01s grab of 4)
#endif
  const uint32_t resident = gridDim.x * (BLOCK / 64);
  uint32_t cur = first, end = first;
#ifndef HRT_GRAB_HEAVY
#define HRT_GRAB_HEAVY 0  // 1: heavy items grabbed kGrab at a time like the others (r03)
#endif
  const uint32_t heavy_end = (HRT_GRAB_HEAVY || !P.items) ? 0u : P.sched[4] * nf;
  unsigned long long cost_sum = 0;
  for (;;) {
    const bool refill = cur >= end;  // wave-uniform
    // (singly, too, while in the plan's heavy prefix: grabbed together, a heavy item's frames queue behind
    // each other on one wave -- HRT_GRAB_HEAVY)
    const uint32_t g = (kargs()->grab_always ||
                        ((uint64_t)cur + (uint64_t)HRT_GRAB_TAIL * resident < n && cur >= heavy_end)) ? kGrab : 1u;
    uint32_t t = 0;
    [[maybe_unused]] unsigned long long qw = 0;
    const KArgs K = kargs();  // (per work item: not held across the item's fused loop)
    if (lane == 0) {
      // a tile's cost: its items' summed clocks; the heavy threshold's sum counts an item by its
      // share of the tile's lanes (its work), so splitting does not raise the threshold (with summed
      // clocks there too, borderline tiles flipped between split and whole: 7.4 / 8.4 ms frames)
      if (prev_tile != 0xFFFFFFFFu) atomicAdd(&K->tile_cost[prev_tile], prev_cost);
      if (refill) {
        if constexpr (Sky)
          qw = atomicAdd(reinterpret_cast<unsigned long long*>(K->sched + kSchedQueue), (unsigned long long)g);
        else
          t = first + atomicAdd(&K->sched[kSchedQueue], g);
      }
    }
    if (prev_tile != 0xFFFFFFFFu) cost_sum += prev_cost >> prev_lk;
    if (refill) {
      if constexpr (Sky) {
        // the front claim (kSchedQueue): bounded by the items trace_sky has taken from the plan's far end
        cur = first + __builtin_amdgcn_readfirstlane((uint32_t)qw);
        const uint32_t back = __builtin_amdgcn_readfirstlane((uint32_t)(qw >> 32));
        const uint32_t sky = K->sky_lane ? min(back, __builtin_amdgcn_readfirstlane(K->sched[kSchedSky]) * nf) : 0u;
        end = min(cur + g, n - sky);
      } else {
        cur = __builtin_amdgcn_readfirstlane(t);
        end = cur + g;
      }
    }
    t = cur;
    if (t >= (Sky ? end : n)) break;  // (Sky: end <= n)
    const uint32_t ti = t / nf, tf = t - ti * nf;
    const uint32_t* items = K->items;
    const uint32_t item = items ? __builtin_amdgcn_readfirstlane(items[ti]) : 0u;
    const uint32_t tile = items ? item & kItemTileMask : ti, lk = (item >> 22) & 7u, sub = (item >> 25) & 63u;
    const bool hot = item >> 31;  // heavy last time: issue priority over the light tiles' waves
    // The grabbed indices of a light item's next frames run as one body (frame runs, trace_fused_split).
    // A heavy item (split, or marked hot) takes its frames one at a time: its pixel chains are the
    // launch's longest, and a run of them in one wave would outlast the launch (runs of 8 frames for
    // every item: island 1.903 -> 2.208 ms per frame, profiles/r04/r04b_ab_island.jsonl).
#ifndef HRT_RUN_HEAVY
#define HRT_RUN_HEAVY 0
#endif
    const uint32_t run = (HRT_FRAME_RUN && (HRT_RUN_HEAVY || (!hot && lk == 0u))) ? min(min(end, n) - t, nf - tf) : 1u;
    cur += run;
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t j = (sub << (6u - lk)) + lane;  // the tile pixel (row-major) of this lane
    uint32_t x = tx * 8 + (j & 7u), lr = ty * 8 + (j >> 3);
    if (lane >= (64u >> lk)) x = 0xFFFFFFFFu;  // idle lane of a split item
    const uint64_t t0 = __builtin_readcyclecounter();
#if HRT_TIMELINE
    const uint64_t rt0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (hot) __builtin_amdgcn_s_setprio(3);
    solo.hot = hot;
    solo.work = 0;
    solo.cache_tile = (HRT_TL_PREPASS && K->tl_cache && lk == 0u) ? tile : 0xFFFFFFFFu;
    body(x, lr, solo, tf, run);
    if (hot) __builtin_amdgcn_s_setprio(0);
#if HRT_TIMELINE
    if (P.timeline && lane == 0) {  // (timeline builds only: the product kernel has no such branch)
      const uint64_t rt1 = __builtin_amdgcn_s_memrealtime();
      const uint32_t slot = atomicAdd(P.timeline_count, 1u);
      if (slot < P.timeline_cap) {
        const uint32_t wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
        P.timeline[4 * (size_t)slot] = rt0;
        P.timeline[4 * (size_t)slot + 1] = solo.t_setup;
        P.timeline[4 * (size_t)slot + 2] = rt1;
        P.timeline[4 * (size_t)slot + 3] = (unsigned long long)(tile | (lk << 22) | (sub << 25) | ((uint32_t)hot << 31)) |
                                           ((unsigned long long)(tf & 0xFFu) << 32) |
                                           ((unsigned long long)(run & 0x7Fu) << 40) |
                                           ((unsigned long long)(solo.t_sky & 1u) << 47) |
                                           ((unsigned long long)(wave & 0xFFFFu) << 48);
      }
    }
#endif
    // cost: the work count where the body keeps one (BUNDLE_CULL_LDS), else shader clocks / 16
    const uint64_t c = CoopOk ? (uint64_t)solo.work : (__builtin_readcyclecounter() - t0) >> 4;
    prev_cost = __builtin_amdgcn_readfirstlane(c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c);
    prev_tile = tile;
    prev_lk = lk;
  }
  if (lane == 0 && prev_tile != 0xFFFFFFFFu) atomicAdd(&P.tile_cost[prev_tile], prev_cost);
  if (prev_tile != 0xFFFFFFFFu) cost_sum += prev_cost >> prev_lk;
  if (lane == 0 && cost_sum) atomicAdd(reinterpret_cast<unsigned long long*>(P.sched + 6), cost_sum);
  add_counters(P, solo.acc_s, solo.acc_t, solo.acc_m);
}

// Planner (after a trace of an LDS variant, before the next).  Items go in decreasing order of the
// tile's last cost (longest first: a long tile started late is what sets a frame's end), by a
// 64-bucket half-octave histogram and a descending scan; heavy tiles are the top buckets: cost >=
// factor x (sum of costs / resident waves), to the bucket, i.e. a tile that alone would take `factor`
// times a wave's fair share of the frame; each runs as 2, 4 or 8 items (bucket_items, <= split_k).  sched[8..71] histogram, [72..135] bucket offsets,
// [136..199] bucket cursors, [3] first heavy bucket.
// The cost buckets, the sched words and a tile's bucket (plan_bucket, its sky rule): hrt_plan.h.
// Both passes count in LDS first: a frame's tiles crowd a few buckets, and per-tile global atomics
// on those few words serialize (0.3 ms per pass at 1080p).
__global__ __launch_bounds__(256) void plan_hist(uint32_t* sched, const uint32_t* cost, uint32_t tiles,
                                                 const uint32_t* tl_cache) {
  __shared__ uint32_t h[kPlanBuckets];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < kPlanBuckets) h[threadIdx.x] = 0;
  __syncthreads();
  if (i < tiles) atomicAdd(&h[plan_bucket(cost, tl_cache, i)], 1u);
  __syncthreads();
  if (threadIdx.x < kPlanBuckets && h[threadIdx.x]) atomicAdd(&sched[kSchedHist + threadIdx.x], h[threadIdx.x]);
}
// factor4: the heavy threshold in quarters of a resident wave's share of the launch's work
__global__ __launch_bounds__(64) void plan_scan(uint32_t* sched, uint32_t waves, uint32_t factor4, uint32_t kmax,
                                                uint32_t prio, uint32_t sky) {
  if (threadIdx.x != 0) return;
  const unsigned long long sum = *reinterpret_cast<const unsigned long long*>(sched + 6);
  const uint32_t hb = cost_bucket((unsigned long long)factor4 * sum / (4ull * (waves ? waves : 1u)));
  uint32_t pos = 0, heavy = 0, heavy_items = 0;
  for (int b = (int)kPlanBuckets - 1; b >= 0; --b) {
    const uint32_t cnt = sched[kSchedHist + b], hv = (uint32_t)b >= hb, k = bucket_items((uint32_t)b, hb, kmax);
    sched[kSchedOff + b] = pos;
    pos += cnt * k;
    heavy += hv ? cnt : 0u;
    heavy_items += hv ? cnt * k : 0u;
  }
  sched[1] = prio > 1 ? heavy_items : pos;  // prio 2: heavy items only (diagnostics)
  sched[2] = heavy;
  sched[4] = heavy_items;  // the plan's first heavy_items items are the heavy tiles' (tile_loop grabs them singly)
  sched[3] = hb;
  // the plan's last items are bucket 0's: the sky tiles, whole and light (not with a heavy bucket 0,
  // whose tiles would be split)
  sched[kSchedSky] = (sky && hb > 0 && prio <= 1) ? sched[kSchedHist] : 0u;
}

// Item word: tile | log2(items of the tile) << 22 | item index s << 25 | heavy << 31 (tile_loop).
__global__ __launch_bounds__(256) void plan_fill(uint32_t* sched, const uint32_t* cost, uint32_t tiles, uint32_t kmax,
                                                 uint32_t prio, uint32_t* items, const uint32_t* tl_cache) {
  __shared__ uint32_t cnt[kPlanBuckets], base[kPlanBuckets];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < kPlanBuckets) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t hb = sched[3];
  const uint32_t b = i < tiles ? plan_bucket(cost, tl_cache, i) : 0u;
  const bool heavy = b >= hb;
  const uint32_t k = bucket_items(b, hb, kmax);
  const uint32_t local = i < tiles ? atomicAdd(&cnt[b], k) : 0u;
  __syncthreads();
  if (threadIdx.x < kPlanBuckets && cnt[threadIdx.x])
    base[threadIdx.x] = sched[kSchedOff + threadIdx.x] + atomicAdd(&sched[kSchedCur + threadIdx.x], cnt[threadIdx.x]);
  __syncthreads();
  if (i >= tiles) return;
  const uint32_t at = base[b] + local;
  if (!heavy) {
    items[at] = i;
  } else {
    const uint32_t flag = prio ? 0x80000000u : 0u;
    if (k == 1) {
      items[at] = i | flag;
    } else {
      const uint32_t lk = (uint32_t)__builtin_ctz(k);
      for (uint32_t s = 0; s < k; ++s) items[at + s] = i | (lk << 22) | (s << 25) | flag;
    }
  }
}

// BUNDLE_CULL with the triangles resident in LDS (bounce survivors are read at LDS rather than L2
// latency).  Dynamic LDS: n_tris x 48 B triangles.
template <int BLOCK, bool D>
__global__ __launch_bounds__(BLOCK) void trace_bundle_cull_lds(TraceParams P) {
  __shared__ uint32_t s_item;
  stage_tris(P, lds_tris, BLOCK);
  // cooperative-tile exchange slots (Coop) after the triangle image, all clear
  unsigned long long* ex = reinterpret_cast<unsigned long long*>(lds_tris + 3 * P.n_tris);
  for (uint32_t k = threadIdx.x; k < 3 * 64; k += BLOCK) ex[k] = ~0ull;
  __syncthreads();
  tile_loop<BLOCK, true>(P, ex, &s_item, [&](uint32_t x, uint32_t lr, Coop& co, uint32_t f, uint32_t nr) {
    trace_fused_split<kBounceCull, D>(P, x, lr, CullLds{lds_tris}, BvhGlobal{}, nullptr, co, f, nr);
  });
}

// BUNDLE_WQ: the hierarchy's nodes in LDS, one pair-stack region per wave after them (persistent
// 1024-thread workgroups).  Dynamic LDS: [nodes x 48 B][16 x (64 slots x 8 B, wq_ncap + wq_tcap words)].
// (one body, two kernels: a __device__ wrapper taking P by reference changes the island kernel's
// register allocation and cost 0.6%)
#define HRT_WQ_KERNEL_BODY(BOUNCE, D, SKY, CAPPED)                                                                 \
  {                                                                                                             \
    const uint32_t nn = P.bvh_wq_n_nodes;                                                                       \
    float4* nodes = lds_tris;                                                                                   \
    for (uint32_t k = threadIdx.x; k < 3 * nn; k += 1024) nodes[k] = P.bvh_wq_nodes[k];                         \
    const uint32_t wave = CAPPED ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6;         \
    char* base = reinterpret_cast<char*>(nodes + 3 * nn) + (size_t)wave * (512 + 4 * (P.wq_ncap + P.wq_tcap));   \
    const WqLds wq{nodes, reinterpret_cast<unsigned long long*>(base), reinterpret_cast<uint32_t*>(base + 512),  \
                   reinterpret_cast<uint32_t*>(base + 512) + P.wq_ncap, P.wq_ncap, CAPPED};                    \
    __syncthreads();                                                                                            \
    const float4* T = reinterpret_cast<const float4*>(P.tris);                                                  \
    tile_loop<1024, false, SKY>(P, nullptr, nullptr, [&](uint32_t x, uint32_t lr, Coop& co, uint32_t f, uint32_t nr) { \
      trace_fused_split<BOUNCE, D>(P, x, lr, CullGlobal{T, to_const(T)}, wq, nullptr, co, f, nr);               \
    });                                                                                                         \
  }
// HRT_WQ_VGPR_CAP: the two kernels' VGPR budget.  Four of their waves per SIMD at 128 VGPRs fill the
// 512-entry file; at 120 they leave 32 registers per lane for a wave of trace_sky beside them.  The cap
// alone cost the traversal 5.7% on island and 1.7% on cave when it was set (36 spilled VGPRs against 14;
// DESIGN §18, profiles/sky_lane_step0.jsonl: 112 + a 64-register trace_sky the same on island, the cap
// dearer on cave; 104: slower), and 3.2% / 2.3% on the tree of DESIGN §20, whose register diet (CAPPED:
// the wave's stack bases in SGPRs, the tile list's length and AABB word made uniform, two addresses formed
// at their use) leaves 15 spilled VGPRs, none of them in the fused sample loop, the pair step, the band
// round or the pool refill, and a cost of 0.4% / 0.4% (profiles/capped_diet_step0.jsonl).
// The diet steers hipcc's allocator (readfirstlane, two empty asm copies) and is a property of the toolchain:
// after a compiler change, run `make asm` and tools/isa_scratch.py and compare the four loops' scratch
// columns with profiles/capped_diet_resources.txt.
// (amdgpu_num_vgpr counts in halves on gfx950: the compiler doubles it for the unified VGPR / AGPR file and
// ignores a value whose double exceeds the launch bounds' 128.)
#ifndef HRT_WQ_VGPR_CAP
#define HRT_WQ_VGPR_CAP 120  // 0: the launch bounds' 128 (no room for trace_sky: HRT_OPT_SKY_LANE then only delays it)
#endif
// Only the <false> instantiations run beside trace_sky: the diagnostics / probe kernels keep the whole
// budget and the plain work counter (explicit specialisations: the attribute takes no template argument).
#if HRT_WQ_VGPR_CAP
#define HRT_WQ_VGPRS __attribute__((amdgpu_num_vgpr(HRT_WQ_VGPR_CAP / 2)))
#else
#define HRT_WQ_VGPRS
#endif
template <bool D>
__global__ void trace_bundle_wq(TraceParams P);
template <>
__global__ __launch_bounds__(1024) HRT_WQ_VGPRS void trace_bundle_wq<false>(TraceParams P) HRT_WQ_KERNEL_BODY(kBounceWq, false, true, true)
template <>
__global__ __launch_bounds__(1024) void trace_bundle_wq<true>(TraceParams P) HRT_WQ_KERNEL_BODY(kBounceWq, true, false, false)
// the same with per-member R in the node margins (TraceParams::bvh_node_r, HRT_OPT_WQ_NODE_RADIUS)
template <bool D>
__global__ void trace_bundle_wq_nr(TraceParams P);
template <>
__global__ __launch_bounds__(1024) HRT_WQ_VGPRS void trace_bundle_wq_nr<false>(TraceParams P) HRT_WQ_KERNEL_BODY(kBounceWqR, false, true, true)
template <>
__global__ __launch_bounds__(1024) void trace_bundle_wq_nr<true>(TraceParams P) HRT_WQ_KERNEL_BODY(kBounceWqR, true, false, false)
// The two kernels for product launches without a sky lane (unplanned launches, HRT_OPT_SKY_LANE off: the
// per-frame loop by default): the whole register budget and the plain work counter -- the cap still costs
// 0.4% where no trace_sky wave uses the registers it frees, and these two keep the code they had (with the
// bases uniform their pair step reads one from a spill lane: 0.9% slower on island).
__global__ __launch_bounds__(1024) void trace_bundle_wq_solo(TraceParams P) HRT_WQ_KERNEL_BODY(kBounceWq, false, false, false)
__global__ __launch_bounds__(1024) void trace_bundle_wq_nr_solo(TraceParams P) HRT_WQ_KERNEL_BODY(kBounceWqR, false, false, false)
#undef HRT_WQ_KERNEL_BODY

// BUNDLE_WQ_L2: the same traversal for hierarchies that do not fit the LDS.  The breadth-first
// image stays in global memory; its first P.wq_lds_nodes slots (the top of the tree: wq_l2_plan) are staged
// into LDS before the stacks.  Dynamic LDS: [wq_lds_nodes x 48 B][16 x (64 slots x 8 B, wq_ncap + wq_tcap words)].
// No sky lane: the _solo shape (the whole register budget, the plain work counter).
#define HRT_WQ_L2_KERNEL_BODY(BOUNCE, D)                                                                         \
  {                                                                                                             \
    const uint32_t nl = P.wq_lds_nodes;                                                                         \
    float4* nodes = lds_tris;                                                                                   \
    for (uint32_t k = threadIdx.x; k < 3 * nl; k += 1024) nodes[k] = P.bvh_wq_nodes_bfs[k];                     \
    const uint32_t wave = threadIdx.x >> 6;                                                                     \
    char* base = reinterpret_cast<char*>(nodes + 3 * nl) + (size_t)wave * (512 + 4 * (P.wq_ncap + P.wq_tcap));   \
    const WqL2 wq{{nodes, reinterpret_cast<unsigned long long*>(base), reinterpret_cast<uint32_t*>(base + 512),  \
                   reinterpret_cast<uint32_t*>(base + 512) + P.wq_ncap, P.wq_ncap, false},                      \
                  (WqGlobalNodes)P.bvh_wq_nodes_bfs, nl};                                                       \
    __syncthreads();                                                                                            \
    const float4* T = reinterpret_cast<const float4*>(P.tris);                                                  \
    tile_loop<1024, false, false>(P, nullptr, nullptr, [&](uint32_t x, uint32_t lr, Coop& co, uint32_t f, uint32_t nr) { \
      trace_fused_split<BOUNCE, D>(P, x, lr, CullGlobal{T, to_const(T)}, wq, nullptr, co, f, nr);               \
    });                                                                                                         \
  }
template <bool D>
__global__ __launch_bounds__(1024) void trace_bundle_wq_l2(TraceParams P) HRT_WQ_L2_KERNEL_BODY(kBounceWqL2, D)
template <bool D>
__global__ __launch_bounds__(1024) void trace_bundle_wq_l2_nr(TraceParams P) HRT_WQ_L2_KERNEL_BODY(kBounceWqL2R, D)
#undef HRT_WQ_L2_KERNEL_BODY

// The sky lane (HRT_OPT_SKY_LANE): the plan's sky items on a lean kernel of their own, resident beside
// the BUNDLE_WQ workgroups -- one more wave per SIMD, which the main kernel's register budget leaves room
// for (HRT_WQ_VGPR_CAP) and which uses no LDS.  The sky loop is pure VALU work; the traversal's waves
// leave issue slots empty while they wait on LDS and L2, and a sky wave in a slot of the main kernel would
// take a traversal wave's place instead.  Each wave takes whole items (a sky tile's remaining frames of
// the launch) from the plan's far end (kSchedQueue) and runs them exactly as trace_fused_split's sky
// branch does: the same sky_samples, seeds, stores, counters and tile costs.  The items are whole-tile,
// light and sky by construction (plan_bucket, plan_scan), so their tile_lists record has an empty list
// and only its octant sums and aabb_ok are read.
#ifndef HRT_SKY_VGPR_CAP
#define HRT_SKY_VGPR_CAP 32
#endif
// Units per back claim: whole items (a tile's 20 frames in one claim) left trace_sky running 0.3 ms after
// the main kernel of a 20-frame launch had ended, and made a rank of 8 slower than without the lane.
#ifndef HRT_SKY_GRAB
#define HRT_SKY_GRAB 4u
#endif
constexpr uint32_t kSkyGrab = HRT_SKY_GRAB;
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(HRT_SKY_VGPR_CAP / 2))) void trace_sky(TraceParams P) {
  if (!P.sky_lane) return;  // (the side stream's warm-up launch, SkyLane::run)
  const uint32_t lane = threadIdx.x & 63;
  const hrt_push_constants& pc = P.pc;
  const uint32_t tiles_x = (pc.width + 7) / 8;
  const uint32_t nf = P.n_frames > 1 ? P.n_frames : 1u;
  // (sky units <= n: bucket 0's tiles, one item each)
  const uint32_t n = P.sched[1] * nf, sky_units = P.sched[kSchedSky] * nf;
  unsigned long long acc_s = 0, acc_t = 0, acc_m = 0, cost_sum = 0;
  uint32_t ran = 0;  // units this wave has run (TraceParams::sky_units)
  __builtin_amdgcn_s_setprio(0);
  uint32_t u = 0, hi = 0;  // the claimed units not yet run: [u, hi)
  for (;;) {
    if (u >= hi) {  // the back claim (kSchedQueue)
      unsigned long long qw = 0;
      if (lane == 0)
        qw = atomicAdd(reinterpret_cast<unsigned long long*>(P.sched + kSchedQueue), (unsigned long long)kSkyGrab << 32);
      const uint32_t front = __builtin_amdgcn_readfirstlane((uint32_t)qw);
      const uint32_t back = __builtin_amdgcn_readfirstlane((uint32_t)(qw >> 32));
      if (back >= sky_units) break;
      hi = n - back;
      u = max(n - min(back + kSkyGrab, sky_units), front);
      if (u >= hi) break;  // the cursors have crossed
    }
    // a frame run: the claimed units of one item (a claim may end one item and begin the next)
    const uint32_t item = u / nf, frame = u - item * nf, nrun = min(hi - u, nf - frame);
    u += nrun;
    ran += nrun;
    const uint32_t tile = __builtin_amdgcn_readfirstlane(P.items[item]) & kItemTileMask;
    const uint64_t t0 = __builtin_readcyclecounter();
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t x = tx * 8 + (lane & 7u), lr = ty * 8 + (lane >> 3);
    const uint32_t y = global_row(lr, P);
    const bool active = x < pc.width && lr < P.local_rows && y < pc.height;
    const uint32_t id = active ? x + y * pc.width : 0u;
    f3 centre = mk(0.0f, 0.0f, 0.0f);
    if (active) {
      const float4 rc = P.rays[id];
      centre = mk(rc.x, rc.y, rc.z);
    }
    const uint32_t* rec = P.tl_cache + (size_t)tile * kTlRecWords;
    TileList tl;
    tl.v = 0;
    tl.lds = nullptr;
    tl.n = 0;
    tl.ok = true;
    tl.aabb = 0;
    tl.tsum = rec[64 + lane];
    tl.aabb_ok = __builtin_amdgcn_readfirstlane(rec[132]) != 0u;
    uint32_t segs = 0, tests = 0;
    f3 colour = mk(0.0f, 0.0f, 0.0f);
    uint32_t state = (pc.rng_offset + frame) * 719393u + id;
    for (uint32_t fr = 0;; ++fr) {
      sky_samples(tl, active, centre, state, colour, segs, tests);
      if (active) store_pixel(P, x, lr, div3(colour, (float)pc.num_samples), frame + fr);
      if (fr + 1u >= nrun) break;
      colour = mk(0.0f, 0.0f, 0.0f);
      state = (pc.rng_offset + frame + fr + 1u) * 719393u + id;
    }
    unsigned long long s, t;
    uint32_t mx;
    wave_counters(segs, tests, s, t, mx);
    acc_s += s;
    acc_t += t;
    acc_m += mx;
    const uint64_t c = (__builtin_readcyclecounter() - t0) >> 4;  // the item's cost, as tile_loop records it
    const uint32_t cost = __builtin_amdgcn_readfirstlane(c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c);
    if (lane == 0) atomicAdd(&P.tile_cost[tile], cost);
    cost_sum += cost;
  }
  if (lane == 0 && cost_sum) atomicAdd(reinterpret_cast<unsigned long long*>(P.sched + 6), cost_sum);
  if (lane == 0 && ran && P.sky_units) atomicAdd(P.sky_units, (unsigned long long)ran);
  add_counters(P, acc_s, acc_t, acc_m);
}

// BUNDLE_BVH with the hierarchy and the triangle image in LDS (persistent 1024-thread workgroups).
// Dynamic LDS: [n_tris x 48 B triangles][nodes x 64 B][prims x 4 B entries][meshes x 4 B key bases].
template <bool D>
__global__ __launch_bounds__(1024) void trace_bundle_bvh_lds(TraceParams P) {
  const uint32_t n = P.n_tris, nn = P.bvh_n_nodes, np = P.bvh_n_prims, nm = P.bvh_n_meshes;
  stage_tris(P, lds_tris, 1024);
  float4* nodes = lds_tris + 3 * n;
  for (uint32_t k = threadIdx.x; k < 4 * nn; k += 1024) nodes[k] = P.bvh_nodes[k];
  uint32_t* entries = reinterpret_cast<uint32_t*>(nodes + 4 * nn);
  for (uint32_t k = threadIdx.x; k < np; k += 1024) entries[k] = P.bvh_entries[k];
  uint32_t* kbase = entries + np;
  for (uint32_t k = threadIdx.x; k < nm; k += 1024) kbase[k] = P.bvh_keybase[k];
  __syncthreads();
  const float4* T = reinterpret_cast<const float4*>(P.tris);
  tile_loop<1024, false>(P, nullptr, nullptr, [&](uint32_t x, uint32_t lr, Coop& co, uint32_t f, uint32_t nr) {
    trace_fused_split<kBounceBvh, D>(P, x, lr, CullGlobal{T, to_const(T)}, BvhLds{nodes, lds_tris, entries, kbase},
                                     nullptr, co, f, nr);
  });
}

// The persistent kernels' whole-tile lists (HRT_TL_PREPASS): one wave per 8x8 tile builds exactly what
// trace_fused_split's build_tile_list would for the tile's whole-tile items (the same pixels, the same
// function) and stores it in the tile's record; the launch's items of the tile then read it back (every
// frame of a multi-frame launch shares the camera and the camera lists).
__global__ __launch_bounds__(256) void tile_lists(TraceParams P, uint32_t refine) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t tiles_x = (P.pc.width + 7) / 8, tiles = tiles_x * ((P.local_rows + 7) / 8);
  const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= tiles) return;  // wave-uniform
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const uint32_t x = tx * 8 + (lane & 7), lr = ty * 8 + (lane >> 3);
  const uint32_t y = global_row(lr, P);
  const bool active = x < P.pc.width && lr < P.local_rows && y < P.pc.height;
  f3 centre = mk(0.0f, 0.0f, 0.0f);
  if (active) {
    const float4 rc = P.rays[x + y * P.pc.width];
    centre = mk(rc.x, rc.y, rc.z);
  }
  const TileList t = build_tile_list(P, active, centre, nullptr, refine != 0u);
  uint32_t* rec = P.tl_cache + (size_t)tile * kTlRecWords;
  rec[lane] = t.v;
  rec[64 + lane] = t.tsum;
  if (lane == 0) {
    rec[128] = t.n;
    rec[129] = t.ok ? 1u : 0u;
    rec[130] = (uint32_t)t.aabb;
    rec[131] = (uint32_t)(t.aabb >> 32);
    rec[132] = t.aabb_ok ? 1u : 0u;
  }
}

// Per-frame prep for the bundle variants: one workgroup per mesh, order-preserving compaction of the
// mesh's camera-facing triangles (num_t(cam_pos) > 0, computed exactly as the trace kernel does).
__global__ __launch_bounds__(256) void camera_lists(TraceParams P) {
  const uint32_t m = blockIdx.x;
  const hrt_mesh& mesh = P.meshes[m];
  __shared__ uint32_t wave_counts[4];
  __shared__ uint32_t base_s;
  uint32_t start = 0;
  for (uint32_t j = 0; j < m; ++j) start += P.meshes[j].len;
  if (threadIdx.x == 0) base_s = 0;
  const f3 o = mk(P.pc.cam_pos[0], P.pc.cam_pos[1], P.pc.cam_pos[2]);
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint32_t c0 = 0; c0 < mesh.len; c0 += 256) {
    const uint32_t k = c0 + threadIdx.x;
    bool keep = false;
    f3 ao = mk(0.0f, 0.0f, 0.0f);
    float nt = 0.0f;
    if (k < mesh.len) {
      const hrt_triangle& t = P.tris[mesh.first_index + k];
      ao = o - ld3(t.a);
      nt = dot(ao, ld3(t.normal));
      keep = nt > 0.0f;
    }
    const unsigned long long ballot = __ballot(keep);
    const uint32_t prefix = __popcll(ballot & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wave_counts[wave] = __popcll(ballot);
    __syncthreads();
    uint32_t off = base_s;
    for (uint32_t w = 0; w < wave; ++w) off += wave_counts[w];
    if (keep) {
      const uint32_t dst = start + off + prefix, idx = mesh.first_index + k;
      const hrt_triangle& t = P.tris[idx];
      const f3 n = ld3(t.normal), e1 = ld3(t.edge_one), e2 = ld3(t.edge_two);
      float4* out = P.cam_tris + 4 * (size_t)dst;
      out[0] = make_float4(ao.x, ao.y, ao.z, nt);
      out[1] = make_float4(e1.x, e1.y, e1.z, __builtin_bit_cast(float, idx));
      out[2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
      out[3] = make_float4(n.x, n.y, n.z, 0.0f);
      // bundle-cull record: the linear forms' coefficients and their margins
      const f3 gu = cross(e2, ao), h = cross(e1, ao);
      const f3 kw = (gu - h) + n;
      auto nrm = [](f3 v) { return __builtin_sqrtf(v.x * v.x + v.y * v.y + v.z * v.z) * 1.0001f; };
      const float pn = nrm(n), pao = nrm(ao), pu = nrm(e2) * pao, pv = nrm(e1) * pao;
      const float tiny = pn * 9.094947017729282e-13f;  // 2^-40 |n|
      float4* cc = P.cam_cull + 5 * (size_t)dst;
      cc[0] = make_float4(n.x, n.y, n.z, 1e-5f * pn);
      cc[1] = make_float4(gu.x, gu.y, gu.z, 1e-5f * pu + tiny);
      cc[2] = make_float4(h.x, h.y, h.z, 1e-5f * pv + tiny);
      cc[3] = make_float4(kw.x, kw.y, kw.z, 1e-5f * (pu + pv + pn) + pn * 6.103515625e-05f);
      cc[4] = make_float4(pn, fmaxf(nrm(gu), pu), fmaxf(nrm(h), pv), nrm(kw) + 1e-5f * (pu + pv + pn));
    }
    __syncthreads();
    if (threadIdx.x == 0) base_s += wave_counts[0] + wave_counts[1] + wave_counts[2] + wave_counts[3];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    P.cam_start[m] = start;
    P.cam_count[m] = base_s;
  }
}

// ---- ray centres (create_ray_subbuffer's loop, src/raytrace_pipeline.rs:319-326) ------------------
// (first + px * x) + py * y per component, each product and sum rounded as written (-ffp-contract=off):
// the same bits as hrt_host_create_rays.
// normalize(triangle normal) once per scene, as resolve_hit would per hit (raytracing.glsl:282 hit_normal)
// One thread per direction cell: the cell's band record (band_cell) -- its list's start and length, then
// the list's first kBandInline entries as half-words (unused ones 0) -- as two 16 B stores.
__global__ __launch_bounds__(256) void band_records(const uint32_t* __restrict__ off, const uint32_t* __restrict__ band16,
                                                    uint4* __restrict__ rec, uint32_t cells) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= cells) return;
  const uint32_t b0 = off[c], n = off[c + 1] - b0;
  uint32_t w[8] = {b0, n, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t j = 0; j < kBandInline; ++j) {
    const uint32_t k = b0 + j;
    if (j < n) w[2 + j / 2] |= ((band16[k >> 1] >> ((k & 1u) << 4)) & 0xFFFFu) << ((j & 1u) << 4);
  }
  rec[2 * (size_t)c] = make_uint4(w[0], w[1], w[2], w[3]);
  rec[2 * (size_t)c + 1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__global__ __launch_bounds__(256) void tri_normals(const hrt_triangle* tris, float4* nhat, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const f3 v = normalize(ld3(tris[i].normal));
  nhat[i] = make_float4(v.x, v.y, v.z, 0.0f);
}

__global__ __launch_bounds__(256) void make_rays(float4* rays, uint32_t width, uint32_t height, float fx, float fy,
                                                 float fz, float pxx, float pxy, float pxz, float pyx, float pyy,
                                                 float pyz) {
  const uint32_t x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= width || y >= height) return;
  const float xf = (float)x, yf = (float)y;
  rays[(size_t)y * width + x] = make_float4((fx + pxx * xf) + pyx * yf, (fy + pxy * xf) + pyy * yf,
                                            (fz + pxz * xf) + pyz * yf, 1.0f);
}

// Self-check of hrt_math.h's shared-reciprocal division and sqrt paths against the compiler's IEEE
// sequences, bit for bit, on hashed inputs (exponents over the whole range for a third of the
// threads, the fast-path range for the rest).  out[0..3]: normalize, div3, sqrt mismatches, fast cases.
__device__ __forceinline__ float math_check_value(uint32_t& st, bool wide) {
  const uint32_t h = hash(st), g = hash(st);
  if (wide) return __builtin_bit_cast(float, h);  // any bit pattern: NaN, inf, denormals, zeros
  const int e = (int)(g % 100u) - 50;             // |v| in [2^-50, 2^50)
  const float m = __builtin_bit_cast(float, 0x3f800000u | (h & 0x007fffffu));
  const float v = __builtin_ldexpf(m, e);
  return (g >> 31) ? -v : v;
}
// Exhaustive over the 2^32 values of a u01 draw (k = base + thread): sqrt_rng against the compiler's
// sqrt on u01(k) and on -2 log(u01(k)), and spec_sincos_angle against spec_sincos on the two angle
// forms of raytracing.glsl (u * 2 * pi and 6.2831852 * u); and adjust_dir's Lambertian shortcut
// premise: a normal_dist radius sqrt(-2 log u) is finite and nonzero iff u is neither 0 nor 1, and the
// cosine of 6.2831852 u is never 0 (and spec_log_u01 equals spec_log on every u01 value); and
// rcp_core's reciprocal is correctly rounded on div_core's range (k read as a float).
// out[0..2]: violations of each.
__global__ __launch_bounds__(256) void math_check_rng(uint32_t base, unsigned long long* out) {
  const uint32_t k = base + blockIdx.x * 256u + threadIdx.x;
  const float u = u01(k);
  const float l = -2.0f * spec_log(u);
  const bool bad_sqrt = fbits(sqrt_rng(u)) != fbits(__builtin_sqrtf(u)) ||
                        fbits(sqrt_rng(l)) != fbits(__builtin_sqrtf(l));
  float s0, c0, s1, c1, s2, c2, s3, c3;
  const float r = (u * 2.0f) * 3.14159265358979323846f, th = 6.2831852f * u;
  spec_sincos(r, s0, c0);
  spec_sincos_angle(r, s1, c1);
  spec_sincos(th, s2, c2);
  spec_sincos_angle(th, s3, c3);
  const bool bad_sc = fbits(s0) != fbits(s1) || fbits(c0) != fbits(c1) || fbits(s2) != fbits(s3) ||
                      fbits(c2) != fbits(c3);
  const float rho = sqrt_rng(l);
  const bool rho_nz = fabsf(rho) < __builtin_inff() && rho != 0.0f;
  const bool bad_fast = rho_nz != (u != 0.0f && u != 1.0f) || c3 == 0.0f ||
                        (k - 1u < 0xFFFFFF7Fu) != (u != 0.0f && u != 1.0f);  // adjust_dir's HRT_FUZZ_INT test
  const bool bad_log = fbits(spec_log_u01(u)) != fbits(spec_log(u));
  // the folded u01 scalings of get_ray_dir and normal_dist (u01_mul), exact by construction
  const bool bad_mul = fbits(u01_mul(k, 3.14159265358979323846f * 0x1p-31f)) != fbits(r) ||
                       fbits(u01_mul(k, 6.2831852f * 0x1p-32f)) != fbits(th);
  if (bad_sqrt) atomicAdd(&out[0], 1ull);
  // the hardware square root alone against the correctly rounded one on both domains (out[3], out[4]):
  // where it never differs, sqrt_rng needs no correction steps
  if (fbits(__builtin_amdgcn_sqrtf(u)) != fbits(__builtin_sqrtf(u))) atomicAdd(&out[3], 1ull);
  if (fbits(__builtin_amdgcn_sqrtf(l)) != fbits(__builtin_sqrtf(l))) atomicAdd(&out[4], 1ull);
  if (bad_sc) atomicAdd(&out[1], 1ull);
  // rcp_core(b) = RN(1/b) for every float b in [2^-40, 2^40] (k read as a float), the premise of
  // div_core's one correction
  const float bk = bitsf(k);
  const bool bad_rcp = bk >= 0x1p-40f && bk <= 0x1p40f && fbits(rcp_core(bk)) != fbits(1.0f / bk);
  if (bad_fast || bad_log || bad_rcp || bad_mul) atomicAdd(&out[2], 1ull);
}
// hrt_debug_band_flatten: BandFlat on 64 given lists (n[l], b0[l]); out[(r * 64 + l) * 2 + {0, 1}] = the
// owner and entry of slot r * 64 + l for each round r < rounds, and out[rounds * 128] = total.
__global__ __launch_bounds__(64) void band_flatten_check(const uint32_t* n_in, const uint32_t* b0_in, uint32_t rounds,
                                                         uint32_t* out) {
  __shared__ uint8_t marks[64];
  const uint32_t lane = threadIdx.x & 63u, n = n_in[lane], b0 = b0_in[lane];
  uint32_t total;
  const uint32_t pos = wave_scan_excl(n, total);  // (the kernel's scan, checked here on given counts)
  BandFlat bf{marks, lane, n, pos, total, b0 - pos, 0u};
  for (uint32_t r = 0; r < rounds; ++r) {
    uint32_t own;
    const uint32_t k = bf.slot(r * 64u, own);
    out[(r * 64u + lane) * 2u] = own;
    out[(r * 64u + lane) * 2u + 1u] = k;
  }
  if (lane == 0) out[rounds * 128u] = total;
}

// hrt_debug_wq_protocol: the pair traversal's LDS handoffs on a scripted run of one wave -- per round,
// the top take[r] entries popped (lane l < take reads entry n - take + l; with take = nn | tn << 8 the
// step's mixed pop, wq_pop: nn node-kind lanes, then tn triangle-kind lanes), each lane's slot read and
// lowering of slot tgt (tgt >= 64: none), then the lanes' pushes (lane l pushes cnt[r][l] <= 4 entries
// (r << 16 | l << 8 | k), slot-major as the node steps push) -- in the product kernel's order, with
// its helpers (wq_push, lds_get, wq_slot_*, wave_handoff).
constexpr uint32_t kProtoCap = 8192;
__global__ __launch_bounds__(64) void wq_protocol_check(uint32_t rounds, const uint32_t* cnt, const uint32_t* take,
                                                        const uint32_t* tgt, const unsigned long long* val,
                                                        const unsigned long long* seed, uint32_t* popped,
                                                        unsigned long long* seen, unsigned long long* slots_out,
                                                        uint32_t* depth_out) {
  __shared__ unsigned long long slot[64];
  __shared__ uint32_t st[kProtoCap];
  const uint32_t lane = threadIdx.x & 63u;
  lds_put(&slot[lane], seed[lane]);
  wave_handoff();
  uint32_t n = 0;
  for (uint32_t r = 0; r < rounds; ++r) {
    // take[r] = nn | tn << 8: the top nn entries to lanes [0, nn) as a step's node pairs, the tn below
    // them to lanes [nn, nn + tn) as its triangle pairs (one stack standing for both: wq_pop's two ranges)
    const uint32_t nn = min(take[r] & 0xFFu, min(n, 64u));
    const uint32_t tn = min(take[r] >> 8, min(n - nn, 64u - nn));
    n -= nn + tn;
    wave_handoff();
    popped[r * 64u + lane] = wq_pop(st, n + tn, nn, st, n, tn, lane, ~0u);
    const uint32_t t = tgt[r * 64u + lane];
    if (t < 64u) {
      seen[r * 64u + lane] = lds_get(&slot[t]);
      wq_slot_lower(slot, t, val[r * 64u + lane]);
    }
    const uint32_t c = cnt[r * 64u + lane];
    wave_handoff();
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) wq_push(st, n, c > k && n + 256u <= kProtoCap, (r << 16) | (lane << 8) | k);
  }
  wave_handoff();
  slots_out[lane] = lds_get(&slot[lane]);
  if (lane == 0) *depth_out = n;
}

__global__ __launch_bounds__(256) void math_check(uint32_t n, uint32_t seed, unsigned long long* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t st = seed * 2654435761u + i;
  const bool wide = (i % 3u) == 0u;
  const f3 a = mk(math_check_value(st, wide), math_check_value(st, wide), math_check_value(st, wide));
  const f3 x = normalize(a), y = normalize_ieee(a);
  const bool bad_n = fbits(x.x) != fbits(y.x) || fbits(x.y) != fbits(y.y) || fbits(x.z) != fbits(y.z);
  const float sv = __builtin_fabsf(math_check_value(st, wide));
  const f3 p = div3(a, sv);
  const bool bad_d = sv > 0.0f && (fbits(p.x) != fbits(a.x / sv) || fbits(p.y) != fbits(a.y / sv) ||
                                   fbits(p.z) != fbits(a.z / sv));
  const float q = __builtin_fabsf(math_check_value(st, wide));
  const bool in = q >= 0x1p-96f && q <= 0x1p80f;
  const bool bad_s = in && fbits(sqrt_core(q)) != fbits(__builtin_sqrtf(q));
  const float d2 = dot(a, a);
  const bool fast = d2 >= 0x1p-80f && d2 <= 0x1p78f;
  if (bad_n) atomicAdd(&out[0], 1ull);
  if (bad_d) atomicAdd(&out[1], 1ull);
  if (bad_s) atomicAdd(&out[2], 1ull);
  if (fast) atomicAdd(&out[3], 1ull);
}

}  // namespace hrt

// ---- launch wrappers (host) ----------------------------------------------------------------------
namespace hrt {

// What a launch's plan reads of its parameters (hrt_launch_plan.h: kernel choice, LDS sizes, splitting).
PlanScene plan_scene(const TraceParams& p) {
  return PlanScene{p.n_tris, p.cam_list_capacity, p.pc.num_meshes, p.pc.max_bounces, p.bvh_nodes != nullptr,
                   p.bvh_entries != nullptr, p.bvh_wq_nodes != nullptr, p.bvh_wq_nodes_bfs != nullptr, p.bvh_sah_milli,
                   p.bvh_n_nodes, p.bvh_n_prims, p.bvh_n_meshes, p.bvh_wq_n_nodes, p.bvh_wq_width, p.bvh_max_leaf,
                   p.bvh_node_r, p.wq_lds_nodes_opt, p.wq_ncap, p.wq_tcap};
}

static uint32_t tiles_of(const TraceParams& p) { return ((p.pc.width + 7) / 8) * ((p.local_rows + 7) / 8); }

// Persistent kernels: plan this trace from the last one's tile costs (when p.plan_valid and
// splitting is on), then reset the counters the trace fills.  q.items = nullptr: plain tile order.
// m: a tile-masked launch (MaskedPlan): always planned, over the selected tiles only, from the lane's costs (read)
// into the context's own sched / item / cost buffers, which the launch then runs from and records into.
static hipError_t prepare_schedule(TraceParams& q, hipStream_t stream, const MaskedPlan* m) {
  // (q.sky_lane: requested by launch_trace; kept only for a planned launch whose work indices and item
  // count leave the queue word's halves apart)
  const uint32_t nf = q.n_frames > 1 ? q.n_frames : 1u;
  const uint32_t tiles = tiles_of(q);
  if (m) {
    if (tiles == 0 || tiles > kItemTileMask || !m->tile_bits || !m->sched || !m->items || !m->cost) return hipErrorInvalidValue;
    if ((uint64_t)tiles * 8u * nf >= (1ull << 31)) q.sky_lane = 0;
    const uint32_t* sky_cache = q.sky_lane ? q.tl_cache : nullptr;
    const uint32_t* cost_in = m->costs_valid ? q.tile_cost : nullptr;
    hipError_t e;
    if ((e = hipMemsetAsync(m->sched + kSchedHist, 0, 3 * kPlanBuckets * 4, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(m->sched + 5, 0, 12, stream)) != hipSuccess) return e;  // (the cost sum the histogram pass adds to)
    if ((e = launch_plan_hist_masked(m->sched, cost_in, m->tile_bits, tiles, sky_cache, stream)) != hipSuccess) return e;
    const uint32_t waves = plan_waves(q.num_cus, nf);
    const uint32_t factor4 = plan_factor4(m->tiles_selected, waves, SplitFactor{q.split_factor, q.split_factor4});
    plan_scan<<<1, 64, 0, stream>>>(m->sched, waves, factor4, q.split_k, q.split_prio, q.sky_lane);
    if ((e = launch_plan_fill_masked(m->sched, cost_in, m->tile_bits, tiles, q.split_k, q.split_prio, m->items, sky_cache,
                                     stream)) != hipSuccess)
      return e;
    q.sched = m->sched;
    q.tile_cost = m->cost;
    q.item_buf = m->items;
    q.items = m->items;
    if ((e = hipMemsetAsync(q.tile_cost, 0, (size_t)tiles * 4, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(q.sched + 5, 0, 12, stream)) != hipSuccess) return e;
    return hipMemsetAsync(q.sched + kSchedQueue, 0, 8, stream);
  }
  // longest-first order whenever last trace's costs are known (and tile indices fit the item word)
  const bool plan = q.plan_valid && tiles > 0 && tiles <= kItemTileMask;
  q.items = plan ? q.item_buf : nullptr;
  if (!plan || (uint64_t)tiles * 8u * nf >= (1ull << 31)) q.sky_lane = 0;
  const uint32_t* sky_cache = q.sky_lane ? q.tl_cache : nullptr;
  hipError_t e;
  if (plan) {
    if ((e = hipMemsetAsync(q.sched + kSchedHist, 0, 3 * kPlanBuckets * 4, stream)) != hipSuccess) return e;  // histogram, cursors
    plan_hist<<<(tiles + 255) / 256, 256, 0, stream>>>(q.sched, q.tile_cost, tiles, sky_cache);
    const uint32_t waves = plan_waves(q.num_cus, nf);
    const uint32_t factor4 = plan_factor4(tiles, waves, SplitFactor{q.split_factor, q.split_factor4});
    plan_scan<<<1, 64, 0, stream>>>(q.sched, waves, factor4, q.split_k, q.split_prio, q.sky_lane);
    plan_fill<<<(tiles + 255) / 256, 256, 0, stream>>>(q.sched, q.tile_cost, tiles, q.split_k, q.split_prio,
                                                       q.item_buf, sky_cache);
  }
  if ((e = hipMemsetAsync(q.tile_cost, 0, (size_t)tiles * 4, stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(q.sched + 5, 0, 12, stream)) != hipSuccess) return e;  // coop counter, cost sum
  return hipMemsetAsync(q.sched + kSchedQueue, 0, 8, stream);  // the work queue word
}

// The persistent kernels' dynamic-LDS limits, set once per device (hrt_create calls this for its device;
// the attribute is per device, so every device a context lives on gets its own call).
// The radiance queries' PAIRS kernel (defined at the end of the file), declared here for the two reasons given
// for query_pairs below -- and AHEAD of it, in this order and in the list's: declared and listed after
// occluded_pairs, its instantiations brought the extra address computation back into the six trace_bundle_wq*,
// the four trace_bundle_wq_l2* and the four query_pairs kernels (profiles/radiance_resources.txt, 5).
template <bool NodeR, bool Stats>
__global__ void radiance_pairs(TraceParams P, RadianceArgs Q);
// The ray queries' PAIRS kernel (defined at the end of the file).  Declared here so that the list below can
// take its instantiations' addresses -- and keep it here: it also fixes where the compiler emits them.  With
// the kernel first used at the end of the file, hipcc compiled the six trace_bundle_wq* kernels' triangle step
// with one more address computation (profiles/query_resources.txt); instantiated from here, every
// pre-existing kernel's code is what it is without the query kernels.
template <bool Primary, bool NodeR>
__global__ void query_pairs(TraceParams P, QueryArgs Q);
// The occlusion queries' PAIRS kernel, declared here for the same two reasons (profiles/occlusion_resources.txt).
template <bool NodeR>
__global__ void occluded_pairs(TraceParams P, QueryArgs Q, uint32_t* bits);
hipError_t ensure_kernel_attributes(int device) {
  static std::mutex mu;
  static std::vector<char> done;
  std::lock_guard<std::mutex> lock(mu);
  if (device < 0) return hipErrorInvalidDevice;
  if ((size_t)device < done.size() && done[(size_t)device]) return hipSuccess;
  // (BUNDLE_CULL_LDS at 512 threads runs two workgroups per CU: lds_block)
  constexpr int kWhole = (int)kMaxLdsScene, kHalf = (int)(kMaxLdsScene / 2);
  const auto fn = [](auto* kernel) { return reinterpret_cast<const void*>(kernel); };
  const std::pair<const void*, int> limits[] = {{fn(&trace_brute_lds), kWhole},
                {fn(&trace_bundle_cull_lds<512, false>), kHalf}, {fn(&trace_bundle_cull_lds<512, true>), kHalf},
                {fn(&trace_bundle_cull_lds<1024, false>), kWhole}, {fn(&trace_bundle_cull_lds<1024, true>), kWhole},
                {fn(&trace_bundle_bvh_lds<false>), kWhole}, {fn(&trace_bundle_bvh_lds<true>), kWhole},
                {fn(&trace_bundle_wq<false>), kWhole}, {fn(&trace_bundle_wq<true>), kWhole},
                {fn(&trace_bundle_wq_nr<false>), kWhole}, {fn(&trace_bundle_wq_nr<true>), kWhole},
                {fn(&trace_bundle_wq_solo), kWhole}, {fn(&trace_bundle_wq_nr_solo), kWhole},
                {fn(&trace_bundle_wq_l2<false>), kWhole}, {fn(&trace_bundle_wq_l2<true>), kWhole},
                {fn(&trace_bundle_wq_l2_nr<false>), kWhole}, {fn(&trace_bundle_wq_l2_nr<true>), kWhole},
                {fn(&radiance_pairs<false, false>), kWhole}, {fn(&radiance_pairs<false, true>), kWhole},
                {fn(&radiance_pairs<true, false>), kWhole}, {fn(&radiance_pairs<true, true>), kWhole},
                {fn(&query_pairs<false, false>), kWhole}, {fn(&query_pairs<false, true>), kWhole},
                {fn(&query_pairs<true, false>), kWhole}, {fn(&query_pairs<true, true>), kWhole},
                {fn(&occluded_pairs<false>), kWhole}, {fn(&occluded_pairs<true>), kWhole}};
  for (const auto& [f, bytes] : limits)
    if (hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); e != hipSuccess)
      return e;
  if (done.size() <= (size_t)device) done.resize((size_t)device + 1, 0);
  done[(size_t)device] = 1;
  return hipSuccess;
}

#ifndef HRT_SKY_GRID
#define HRT_SKY_GRID 1u  // trace_sky workgroups per CU
#endif
hipError_t launch_trace(const TraceParams& p0, const LaunchPlan& plan, hipStream_t stream, const SkyLane* sky,
                        const MaskedPlan* masked) {
  TraceParams p = p0;
  const int k = plan.kernel;
  const KernelTraits& kt = kernel_traits(k);
  p.sec_batch = batch_threshold(p.sec_batch, plan.sec_batch);
  p.prim_batch = batch_threshold(p.prim_batch, plan.prim_batch);
  if (kt.camera_lists && p.pc.num_meshes > 0 && !p.cam_lists_ready) camera_lists<<<p.pc.num_meshes, 256, 0, stream>>>(p);
  if (masked && (!kt.persistent || p0.diag || p0.probe)) return hipErrorInvalidValue;  // (the caller falls back to whole frames)
  if (!kt.persistent) {
    const int px = plan.block == 1024 ? 32 : 16;  // a workgroup's square of pixels
    const dim3 grid((p.pc.width + px - 1) / px, (p.local_rows + px - 1) / px, 1);
    void (*kernel)(TraceParams) =
        k == HRT_KERNEL_LITERAL       ? trace_literal
        : k == HRT_KERNEL_BRUTE_LDS   ? trace_brute_lds
        : k == HRT_KERNEL_BUNDLE      ? (p.diag ? trace_bundle<true> : trace_bundle<false>)
        : k == HRT_KERNEL_BUNDLE_CULL ? (p.diag ? trace_bundle_cull<true> : trace_bundle_cull<false>)
        : k == HRT_KERNEL_BUNDLE_BVH  ? (p.diag ? trace_bundle_bvh<true> : trace_bundle_bvh<false>)
                                      : trace_brute;
    kernel<<<grid, plan.block, plan.lds_bytes, stream>>>(p);
    return hipGetLastError();
  }
  // The persistent kernels: tile lists, this launch's scheduling parameters, the planner, then the kernel
  if (HRT_TL_PREPASS && p.tl_cache && !p.tl_lists_ready) tile_lists<<<(tiles_of(p) + 3) / 4, 256, 0, stream>>>(p, 1u);
  TraceParams q = p;
  if (q.split_k == 0) q.split_k = plan.split_k;
  // (BUNDLE_CULL_LDS's split_k 1: cooperative heavy tiles instead)
  q.coop = k == HRT_KERNEL_BUNDLE_CULL_LDS && p.coop && q.split_k == 1 && p.pc.num_meshes <= 62;
  if (kt.pair_traversal) {
    const SplitFactor f = pair_split(tiles_of(p), p.n_frames, p.num_cus, q.split_factor);
    q.split_factor = f.factor;
    q.split_factor4 = f.factor4;
    q.wq_ncap = plan.wq_ncap;
    q.wq_tcap = plan.wq_tcap;
    q.wq_lds_nodes = plan.wq_lds_nodes;
  }
  // The sky lane: product kernels only (diagnostics, probes and timeline builds keep every item on the
  // main kernel), a scene without spheres (trace_fused_split's sky rule) and a planned launch
  // (prepare_schedule).  The side stream waits for the planner kernels; the main stream waits for
  // trace_sky before anything that follows this launch.
  const bool d = p.diag || p.probe;
  q.sky_lane = kt.sky_lane && sky && sky->run && !HRT_TIMELINE && HRT_TL_PREPASS && HRT_SKY_LOOP && !d && p.tl_cache &&
               p.pc.num_spheres == 0;
  if (hipError_t e = prepare_schedule(q, stream, masked); e != hipSuccess) return e;
  if (q.sky_lane) {
    if (hipError_t e = hipEventRecord(sky->fork, stream); e != hipSuccess) return e;
    if (hipError_t e = hipStreamWaitEvent(sky->stream, sky->fork, 0); e != hipSuccess) return e;
  }
  const bool nr = p.bvh_node_r != 0, lane = q.sky_lane != 0;  // (BUNDLE_WQ without the lane: the kernels outside the register cap)
  void (*kernel)(TraceParams) =
      k == HRT_KERNEL_BUNDLE_BVH_LDS ? (d ? trace_bundle_bvh_lds<true> : trace_bundle_bvh_lds<false>)
      : k == HRT_KERNEL_BUNDLE_WQ && nr ? (d ? trace_bundle_wq_nr<true> : lane ? trace_bundle_wq_nr<false> : trace_bundle_wq_nr_solo)
      : k == HRT_KERNEL_BUNDLE_WQ       ? (d ? trace_bundle_wq<true> : lane ? trace_bundle_wq<false> : trace_bundle_wq_solo)
      : k == HRT_KERNEL_BUNDLE_WQ_L2 && nr ? (d ? trace_bundle_wq_l2_nr<true> : trace_bundle_wq_l2_nr<false>)
      : k == HRT_KERNEL_BUNDLE_WQ_L2       ? (d ? trace_bundle_wq_l2<true> : trace_bundle_wq_l2<false>)
      : plan.block == 512 ? (d ? trace_bundle_cull_lds<512, true> : trace_bundle_cull_lds<512, false>)  // BUNDLE_CULL_LDS
                          : (d ? trace_bundle_cull_lds<1024, true> : trace_bundle_cull_lds<1024, false>);
  kernel<<<plan.groups_per_cu * p.num_cus, plan.block, plan.lds_bytes, stream>>>(q);
  if (q.sky_lane) {
    // (after the main kernel's launch: its workgroups take their CUs first, one sky workgroup fits beside each)
    trace_sky<<<p.num_cus * HRT_SKY_GRID, 256, 0, sky->stream>>>(q);
    if (hipError_t e = hipEventRecord(sky->join, sky->stream); e != hipSuccess) return e;
    if (hipError_t e = hipStreamWaitEvent(stream, sky->join, 0); e != hipSuccess) return e;
  } else if (sky && !sky->run) {
    trace_sky<<<1, 256, 0, sky->stream>>>(q);  // (returns at once: q.sky_lane == 0; nothing to order)
  }
  return hipGetLastError();
}

hipError_t launch_tile_lists(const TraceParams& p, uint32_t refine, hipStream_t stream) {
  if (!p.tl_cache) return hipErrorInvalidValue;
  if (p.pc.num_meshes > 0) camera_lists<<<p.pc.num_meshes, 256, 0, stream>>>(p);
  tile_lists<<<(tiles_of(p) + 3) / 4, 256, 0, stream>>>(p, refine);
  return hipGetLastError();
}

hipError_t launch_make_rays(float4* rays, uint32_t width, uint32_t height, const float first[3], const float px[3],
                            const float py[3], hipStream_t stream) {
  if (width == 0 || height == 0) return hipSuccess;
  const dim3 g((width + 15) / 16, (height + 15) / 16, 1);
  make_rays<<<g, 256, 0, stream>>>(rays, width, height, first[0], first[1], first[2], px[0], px[1], px[2], py[0],
                                   py[1], py[2]);
  return hipGetLastError();
}

hipError_t launch_band_records(const uint32_t* off, const uint32_t* band16, uint32_t* rec, uint32_t cells,
                               hipStream_t stream) {
  if (cells == 0) return hipSuccess;
  band_records<<<(cells + 255) / 256, 256, 0, stream>>>(off, band16, reinterpret_cast<uint4*>(rec), cells);
  return hipGetLastError();
}

hipError_t launch_tri_normals(const hrt_triangle* tris, float4* nhat, uint32_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  tri_normals<<<(n + 255) / 256, 256, 0, stream>>>(tris, nhat, n);
  return hipGetLastError();
}

hipError_t launch_wq_protocol_check(uint32_t rounds, const uint32_t* cnt, const uint32_t* take, const uint32_t* tgt,
                                    const unsigned long long* val, const unsigned long long* seed, uint32_t* popped,
                                    unsigned long long* seen, unsigned long long* slots, uint32_t* depth,
                                    hipStream_t stream) {
  wq_protocol_check<<<1, 64, 0, stream>>>(rounds, cnt, take, tgt, val, seed, popped, seen, slots, depth);
  return hipGetLastError();
}
hipError_t launch_band_flatten_check(const uint32_t* n, const uint32_t* b0, uint32_t rounds, uint32_t* out,
                                     hipStream_t stream) {
  band_flatten_check<<<1, 64, 0, stream>>>(n, b0, rounds, out);
  return hipGetLastError();
}
hipError_t launch_math_check_rng(unsigned long long* out, hipStream_t stream) {
  for (uint64_t base = 0; base < (1ull << 32); base += (1ull << 28)) {  // 16 launches of 2^28 states
    math_check_rng<<<(1u << 28) / 256u, 256, 0, stream>>>((uint32_t)base, out);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_math_check(uint32_t n, uint32_t seed, unsigned long long* out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  math_check<<<(n + 255) / 256, 256, 0, stream>>>(n, seed, out);
  return hipGetLastError();
}

// ---- ray queries: closest hit of caller rays and of un-jittered primary rays -------------
// One ray per lane.  A query is the reference's world_hit (raytracing.glsl:267-288) for one ray that did not
// come from a pixel's sample chain; the three methods feed it to world_hit's three
// implementations above and give the same bytes:
//   SCAN   the statement-by-statement scan, its running closest seeded with the ray's t_max;
//   BVH    world_hit_bounce_bvh on the global-memory hierarchy (irregular list and grazing band included);
//   PAIRS  world_hit_bounce_wq, 64 rays per wave, the node image in LDS (persistent 1024-thread workgroups).
// The traversals start their closest at FLT_MAX (spheres_first), so t_max is applied to their result: the
// closest accepted hit overall, first in scan order among equals, is the seeded scan's answer when it lies
// below t_max, and otherwise nothing the scan accepts does.  A ray whose origin or normalised direction is
// not finite, or whose direction's squared length is zero, denormal or overflows (its quotient is then no
// unit vector), is outside the traversals' analysis and takes the scan whatever the method.
struct QueryRay {
  f3 o, d;     // origin, S4-normalised direction
  float best;  // min(t_max, FLT_MAX): where the running closest starts
  bool live;   // a ray of the launch that is not a certain miss (t_max > 0.001, not NaN)
  bool finite; // every component of o and d is finite and d is a unit vector (dot(v, v) normal and finite)
};
__device__ __forceinline__ bool finite3(f3 a) {
  return fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff();
}
template <bool Primary>
__device__ __forceinline__ QueryRay query_ray(const TraceParams& P, const QueryArgs& Q, uint32_t i) {
  QueryRay r{mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 1.0f), kFltMax, false, true};
  if (i >= Q.n) return r;
  float t_max = kFltMax;
  f3 v;
  if constexpr (Primary) {
    const uint32_t k = Q.first + i, x = Q.x0 + k % Q.w, y = Q.y0 + k / Q.w;
    const float4 rc = P.rays[x + (size_t)y * P.pc.width];
    const float* M = P.pc.cam_alignment_mat;
    // mat3(M) c, row-wise as get_ray_dir spells it
    v = mk(__builtin_fmaf(M[8], rc.z, __builtin_fmaf(M[4], rc.y, M[0] * rc.x)),
           __builtin_fmaf(M[9], rc.z, __builtin_fmaf(M[5], rc.y, M[1] * rc.x)),
           __builtin_fmaf(M[10], rc.z, __builtin_fmaf(M[6], rc.y, M[2] * rc.x)));
    r.o = mk(P.pc.cam_pos[0], P.pc.cam_pos[1], P.pc.cam_pos[2]);
  } else {
    const float4 a = Q.rays[2 * (size_t)i], b = Q.rays[2 * (size_t)i + 1];
    r.o = mk(a.x, a.y, a.z);
    t_max = a.w;
    v = mk(b.x, b.y, b.z);
  }
  r.d = normalize(v);
  r.live = t_max > 0.001f;  // (false for NaN)
  r.best = t_max > kFltMax ? kFltMax : t_max;
  // (a zero, denormal or overflowed dot(v, v) leaves a d that is finite at best, not a unit vector)
  const float d2 = dot(v, v);
  r.finite = finite3(r.o) && finite3(r.d) && d2 >= 0x1p-126f && d2 <= kFltMax;
  return r;
}

// world_hit_literal with the running closest started at `best` and the given counts.
__device__ __forceinline__ Closest world_hit_scan_from(const Scene& sc, int n_spheres, int n_meshes, f3 o, f3 d,
                                                       float best, uint32_t& tests) {
  Closest c{best, 0, 0u, 0u};
  for (int i = 0; i < n_spheres; ++i) {
    const float t = sphere_dist(sc.spheres[i], o, d);
    if (t > 0.001f && t < c.t) c = Closest{t, 1, (uint32_t)i, 0u};
  }
  for (int m = 0; m < n_meshes; ++m) {
    const hrt_mesh& mesh = sc.meshes[m];
    if (!aabb_pass(mesh, o, d)) continue;
    tests += mesh.len;
    const uint32_t end = mesh.first_index + mesh.len;
    for (uint32_t i = mesh.first_index; i < end; ++i) {
      float t;
      if (tri_accept_exact(sc.tris[i], o, d, c.t, t)) c = Closest{t, 2, i, (uint32_t)m};
    }
  }
  return c;
}

// The hit record of ray i (two 16-byte vector stores) and the wave's share of the statistics.  ALL 64 lanes.
__device__ __forceinline__ void query_store(const Scene& sc, const QueryArgs& Q, uint32_t i, const QueryRay& r,
                                            const Closest& c, uint32_t tests) {
  if (i < Q.n) {
    float4 h0 = make_float4(kFltMax, bitsf(0u), bitsf(0xFFFFFFFFu), bitsf(0xFFFFFFFFu));
    float4 h1 = make_float4(0.0f, 0.0f, 0.0f, bitsf(0u));
    if (c.kind != 0) {
      const HitRecord h = resolve_hit(sc, c, r.o, r.d);
      h0 = make_float4(c.t, bitsf((uint32_t)c.kind), bitsf(c.idx), bitsf(c.kind == 2 ? c.mesh : 0xFFFFFFFFu));
      h1 = make_float4(h.normal.x, h.normal.y, h.normal.z, bitsf(0u));
    }
    Q.hits[2 * (size_t)i] = h0;
    Q.hits[2 * (size_t)i + 1] = h1;
  }
  if (Q.stats) {
    unsigned long long s = (r.live && !r.finite) ? 1u : 0u, t = tests;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_xor(s, off, 64);
      t += __shfl_xor(t, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && (s | t)) {
      if (s) atomicAdd(&Q.stats[0], s);
      if (t) atomicAdd(&Q.stats[1], t);
    }
  }
}

template <bool Primary>
__global__ __launch_bounds__(256) void query_scan(TraceParams P, QueryArgs Q) {
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const QueryRay r = query_ray<Primary>(P, Q, i);
  uint32_t tests = 0;
  Closest c{kFltMax, 0, 0u, 0u};
  if (r.live) c = world_hit_scan_from(sc, P.pc.num_spheres, P.pc.num_meshes, r.o, r.d, r.best, tests);
  query_store(sc, Q, i, r, c, tests);
}

// a traversal's result under t_max, or the literal scan of a ray outside the traversals' domain
__device__ __forceinline__ void query_finish(const Scene& sc, const TraceParams& P, const QueryRay& r, bool trav,
                                             Closest& c, uint32_t& tests) {
  if (!trav || !(c.t < r.best)) c = Closest{kFltMax, 0, 0u, 0u};
  if (r.live && !r.finite) c = world_hit_scan_from(sc, P.pc.num_spheres, P.pc.num_meshes, r.o, r.d, r.best, tests);
}

template <bool Primary>
__global__ __launch_bounds__(256) void query_bvh(TraceParams P, QueryArgs Q) {
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const QueryRay r = query_ray<Primary>(P, Q, i);
  const bool trav = r.live && r.finite;
  const f3 o = trav ? r.o : mk(0.0f, 0.0f, 0.0f), d = trav ? r.d : mk(0.0f, 0.0f, 1.0f);
  uint32_t tests = 0;
  Closest c{kFltMax, 0, 0u, 0u};
  Diag dg;
  world_hit_bounce_bvh<false>(sc, P, BvhGlobal{P.bvh_nodes, P.bvh_prims}, trav, o, d, tests, c, dg);
  query_finish(sc, P, r, trav, c, tests);
  query_store(sc, Q, i, r, c, tests);
}

// PAIRS: the node image staged into LDS and the per-wave stacks carved as the BUNDLE_WQ kernels carve them;
// each wave then takes 64 rays at a time (all 64 lanes enter the traversal, tail lanes as inactive rays).
template <bool Primary, bool NodeR>
__global__ __launch_bounds__(1024) void query_pairs(TraceParams P, QueryArgs Q) {
  const uint32_t nn = P.bvh_wq_n_nodes;
  float4* nodes = lds_tris;
  for (uint32_t k = threadIdx.x; k < 3 * nn; k += 1024) nodes[k] = P.bvh_wq_nodes[k];
  const uint32_t wave = threadIdx.x >> 6;
  char* base = reinterpret_cast<char*>(nodes + 3 * nn) + (size_t)wave * (512 + 4 * (P.wq_ncap + P.wq_tcap));
  const WqLds wq{nodes, reinterpret_cast<unsigned long long*>(base), reinterpret_cast<uint32_t*>(base + 512),
                 reinterpret_cast<uint32_t*>(base + 512) + P.wq_ncap, P.wq_ncap, false};
  __syncthreads();
  // (wave-uniform trip count: i - lane is the wave's first ray)
  for (uint32_t w0 = blockIdx.x * 1024u + wave * 64u; w0 < Q.n; w0 += gridDim.x * 1024u) {
    const uint32_t i = w0 + (threadIdx.x & 63u);
    const QueryRay r = query_ray<Primary>(P, Q, i);
    const bool trav = r.live && r.finite;
    const f3 o = trav ? r.o : mk(0.0f, 0.0f, 0.0f), d = trav ? r.d : mk(0.0f, 0.0f, 1.0f);
    uint32_t tests = 0;
    Closest c{kFltMax, 0, 0u, 0u};
    Diag dg;
    world_hit_bounce_wq<false, NodeR>(kscene(), P, wq, trav, o, d, tests, c, dg);
    const Scene sc = kscene();
    query_finish(sc, P, r, trav, c, tests);
    query_store(sc, Q, i, r, c, tests);
  }
}

hipError_t launch_query(const TraceParams& p0, const QueryArgs& q, const QueryPlan& plan, bool primary,
                        hipStream_t stream) {
  if (q.n == 0) return hipSuccess;
  const uint32_t blocks = (q.n + 255u) / 256u;
  switch (plan.method) {
    case HRT_QUERY_SCAN:
      primary ? query_scan<true><<<blocks, 256, 0, stream>>>(p0, q) : query_scan<false><<<blocks, 256, 0, stream>>>(p0, q);
      break;
    case HRT_QUERY_BVH:
      primary ? query_bvh<true><<<blocks, 256, 0, stream>>>(p0, q) : query_bvh<false><<<blocks, 256, 0, stream>>>(p0, q);
      break;
    case HRT_QUERY_PAIRS: {
      if (plan.lds_bytes == 0) return hipErrorInvalidValue;
      TraceParams p = p0;
      p.wq_ncap = plan.wq_ncap;
      p.wq_tcap = plan.wq_tcap;
      // (their dynamic-LDS limit: ensure_kernel_attributes)
      void (*kernel)(TraceParams, QueryArgs) =
          p.bvh_node_r ? (primary ? query_pairs<true, true> : query_pairs<false, true>)
                       : (primary ? query_pairs<true, false> : query_pairs<false, false>);
      const uint32_t groups = std::min((q.n + 1023u) / 1024u, std::max(1u, p.num_cus));
      kernel<<<groups, 1024, plan.lds_bytes, stream>>>(p, q);
      break;
    }
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ---- occlusion queries: any hit of caller rays, one bit per ray -------------------
// occluded(i) = (the query above, same ray and method, returns kind != 0).  One ray per lane; a wave owns 64
// consecutive rays whose first index is a multiple of 64, and so two words of the output: it forms them with
// a ballot, and lanes 0 and 1 store one each (a word is written iff its first ray is below n; rays past n
// contribute 0 bits).  The three methods:
//   SCAN   world_hit_scan_from(...).kind != 0 -- the yardstick, no early exit;
//   BVH    world_hit_bounce_bvh over BvhGlobalAny: closest seeded with the ray's best, lanes leave at a hit;
//   PAIRS  world_hit_bounce_wq over WqLdsAny: slot seeded with best, lowered to +0 at a hit.
// Exactness: every cull proves "the scan rejects this triangle given a running closest of c";
// the seeded scan's running closest never exceeds best, so until a hit is found nothing with 0.001 < dist <
// best behind its mesh's gate is culled, and after one the answer is 1 whatever else is skipped.
// ALL 64 lanes.
__device__ __forceinline__ void occluded_store(const QueryArgs& Q, uint32_t* bits, uint32_t i, const QueryRay& r,
                                               bool occ, uint32_t tests) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long b = __ballot(occ && i < Q.n);
  const uint32_t first = (i - lane) + 32u * lane;  // lanes 0, 1: the first ray of the wave's two words
  if (lane < 2u && first < Q.n) bits[first >> 5] = (uint32_t)(b >> (32u * lane));
  if (Q.stats) {
    unsigned long long s = (r.live && !r.finite) ? 1u : 0u, t = tests;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_xor(s, off, 64);
      t += __shfl_xor(t, off, 64);
    }
    if (lane == 0 && (s | t | b)) {
      if (s) atomicAdd(&Q.stats[0], s);
      if (t) atomicAdd(&Q.stats[1], t);
      if (b) atomicAdd(&Q.stats[2], (unsigned long long)__popcll(b));
    }
  }
}

__global__ __launch_bounds__(256) void occluded_scan(TraceParams P, QueryArgs Q, uint32_t* bits) {
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const QueryRay r = query_ray<false>(P, Q, i);
  uint32_t tests = 0;
  bool occ = false;
  if (r.live) occ = world_hit_scan_from(sc, P.pc.num_spheres, P.pc.num_meshes, r.o, r.d, r.best, tests).kind != 0;
  occluded_store(Q, bits, i, r, occ, tests);
}

// a traversal's answer, or the literal scan's for a ray outside the traversals' domain
__device__ __forceinline__ bool occluded_finish(const Scene& sc, const TraceParams& P, const QueryRay& r, bool trav,
                                                const Closest& c, uint32_t& tests) {
  if (r.live && !r.finite)
    return world_hit_scan_from(sc, P.pc.num_spheres, P.pc.num_meshes, r.o, r.d, r.best, tests).kind != 0;
  return trav && c.kind != 0;
}

__global__ __launch_bounds__(256) void occluded_bvh(TraceParams P, QueryArgs Q, uint32_t* bits) {
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const QueryRay r = query_ray<false>(P, Q, i);
  const bool trav = r.live && r.finite;
  const f3 o = trav ? r.o : mk(0.0f, 0.0f, 0.0f), d = trav ? r.d : mk(0.0f, 0.0f, 1.0f);
  uint32_t tests = 0;
  Closest c{r.best, 0, 0u, 0u};  // (the seed: BvhGlobalAny)
  Diag dg;
  world_hit_bounce_bvh<false>(sc, P, BvhGlobalAny{{P.bvh_nodes, P.bvh_prims}}, trav, o, d, tests, c, dg);
  const bool occ = occluded_finish(sc, P, r, trav, c, tests);
  occluded_store(Q, bits, i, r, occ, tests);
}

// PAIRS: carved exactly as query_pairs.
template <bool NodeR>
__global__ __launch_bounds__(1024) void occluded_pairs(TraceParams P, QueryArgs Q, uint32_t* bits) {
  const uint32_t nn = P.bvh_wq_n_nodes;
  float4* nodes = lds_tris;
  for (uint32_t k = threadIdx.x; k < 3 * nn; k += 1024) nodes[k] = P.bvh_wq_nodes[k];
  const uint32_t wave = threadIdx.x >> 6;
  char* base = reinterpret_cast<char*>(nodes + 3 * nn) + (size_t)wave * (512 + 4 * (P.wq_ncap + P.wq_tcap));
  const WqLdsAny wq{{nodes, reinterpret_cast<unsigned long long*>(base), reinterpret_cast<uint32_t*>(base + 512),
                     reinterpret_cast<uint32_t*>(base + 512) + P.wq_ncap, P.wq_ncap, false}};
  __syncthreads();
  // (wave-uniform trip count: i - lane is the wave's first ray, a multiple of 64)
  for (uint32_t w0 = blockIdx.x * 1024u + wave * 64u; w0 < Q.n; w0 += gridDim.x * 1024u) {
    const uint32_t i = w0 + (threadIdx.x & 63u);
    const QueryRay r = query_ray<false>(P, Q, i);
    const bool trav = r.live && r.finite;
    const f3 o = trav ? r.o : mk(0.0f, 0.0f, 0.0f), d = trav ? r.d : mk(0.0f, 0.0f, 1.0f);
    uint32_t tests = 0;
    Closest c{r.best, 0, 0u, 0u};  // (the seed: WqLdsAny)
    Diag dg;
    world_hit_bounce_wq<false, NodeR>(kscene(), P, wq, trav, o, d, tests, c, dg);
    const Scene sc = kscene();
    const bool occ = occluded_finish(sc, P, r, trav, c, tests);
    occluded_store(Q, bits, i, r, occ, tests);
  }
}

hipError_t launch_occluded(const TraceParams& p0, const QueryArgs& q, uint32_t* bits, const QueryPlan& plan,
                           hipStream_t stream) {
  if (q.n == 0) return hipSuccess;
  const uint32_t blocks = (q.n + 255u) / 256u;
  switch (plan.method) {
    case HRT_QUERY_SCAN:
      occluded_scan<<<blocks, 256, 0, stream>>>(p0, q, bits);
      break;
    case HRT_QUERY_BVH:
      occluded_bvh<<<blocks, 256, 0, stream>>>(p0, q, bits);
      break;
    case HRT_QUERY_PAIRS: {
      if (plan.lds_bytes == 0) return hipErrorInvalidValue;
      TraceParams p = p0;
      p.wq_ncap = plan.wq_ncap;
      p.wq_tcap = plan.wq_tcap;
      // (their dynamic-LDS limit: ensure_kernel_attributes)
      void (*kernel)(TraceParams, QueryArgs, uint32_t*) = p.bvh_node_r ? occluded_pairs<true> : occluded_pairs<false>;
      const uint32_t groups = std::min((q.n + 1023u) / 1024u, std::max(1u, p.num_cus));
      kernel<<<groups, 1024, plan.lds_bytes, stream>>>(p, q, bits);
      break;
    }
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ---- radiance queries: the reference's main() for caller records ------------------
// out[i] = (sum over num_samples of trace_ray(origin, normalize(get_ray_dir(pc, centre, state)), state) /
// num_samples, 1.0) with state started at the record's seed: a pixel of a frame is the record (cam_pos,
// rng_offset * 719393 + id, ray centre id).  One query per lane.  Every SEGMENT takes S11's test -- origin
// finite, direction finite with dot(d, d) normal and finite -- and one that fails it is answered by the literal
// scan whatever the method (stats[0]); the three methods feed the others to world_hit's three implementations:
//   SCAN   trace_literal's loops over world_hit_scan_from and shade_step -- the yardstick;
//   BVH    the same loop wave-converged, one world_hit_bounce_bvh per trip;
//   PAIRS  trace_fused_split's loop without tile lists: every segment through world_hit_bounce_wq, shading in
//          two phases, lanes refilled from one grid-wide query counter.
// A query's result is a function of its record alone (its own RNG chain, its samples in order), so which lane
// or wave runs it, and in whose company, cannot show in the bytes.
struct RadianceRecord {
  f3 origin, centre;
  uint32_t seed;
};
__device__ __forceinline__ RadianceRecord radiance_record(const RadianceArgs& Q, uint32_t i) {
  const float4 a = Q.queries[2 * (size_t)i], b = Q.queries[2 * (size_t)i + 1];
  return RadianceRecord{mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), fbits(a.w)};
}
// S11's test of one segment (d: the direction the segment is traced with)
__device__ __forceinline__ bool segment_regular(f3 o, f3 d) {
  const float d2 = dot(d, d);
  return finite3(o) && finite3(d) && d2 >= 0x1p-126f && d2 <= kFltMax;
}
// The wave's share of the call's three counts: one atomic each.  ALL 64 lanes.
__device__ __forceinline__ void radiance_counts(unsigned long long* stats, uint32_t scan, uint32_t segs, uint32_t tests) {
  if (!stats) return;
  unsigned long long s, t, a = scan;
  uint32_t mx;
  wave_counters(segs, tests, s, t, mx);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
  if ((threadIdx.x & 63u) == 0) {
    if (a) atomicAdd(&stats[0], a);
    if (s) atomicAdd(&stats[1], s);
    if (t) atomicAdd(&stats[2], t);
  }
}

__global__ __launch_bounds__(256) void radiance_scan(TraceParams P, RadianceArgs Q) {
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  const hrt_push_constants& pc = P.pc;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t scan = 0, segs = 0, tests = 0;
  if (i < Q.n) {
    const RadianceRecord q = radiance_record(Q, i);
    f3 colour = mk(0.0f, 0.0f, 0.0f);
    uint32_t state = q.seed;
    for (int s = 0; s < pc.num_samples; ++s) {
      const f3 dir = get_ray_dir(pc, q.centre, state);
      Path p{mk(0.0f, 0.0f, 0.0f), mk(1.0f, 1.0f, 1.0f), q.origin, normalize(dir), 0, true};
      for (int b = 0; b <= pc.max_bounces; ++b) {
        if (!segment_regular(p.pos, p.dir)) ++scan;
        const Closest c = world_hit_scan_from(sc, pc.num_spheres, pc.num_meshes, p.pos, p.dir, kFltMax, tests);
        ++segs;
        if (shade_step(sc, pc, p, c, state)) break;
      }
      colour = colour + p.light * p.colour;
    }
    colour = div3(colour, (float)pc.num_samples);
    Q.out[i] = make_float4(colour.x, colour.y, colour.z, 1.0f);
  }
  radiance_counts(Q.stats, scan, segs, tests);
}

__global__ __launch_bounds__(256) void radiance_bvh(TraceParams P, RadianceArgs Q) {
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  const hrt_push_constants& pc = P.pc;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool live = i < Q.n;
  RadianceRecord q{mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.0f), 0u};
  if (live) q = radiance_record(Q, i);
  uint32_t scan = 0, segs = 0, tests = 0;
  f3 colour = mk(0.0f, 0.0f, 0.0f);
  uint32_t state = q.seed;
  int sample = 0;
  Path p{mk(0.0f, 0.0f, 0.0f), mk(1.0f, 1.0f, 1.0f), mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 1.0f), 0, true};
  p.bounce = pc.max_bounces + 1;  // no path under way
  bool done = !live;
  while (__any(!done)) {
    if (!done && p.bounce > pc.max_bounces) {
      if (sample >= pc.num_samples) {
        done = true;
      } else {
        ++sample;
        const f3 dir = get_ray_dir(pc, q.centre, state);
        p = Path{mk(0.0f, 0.0f, 0.0f), mk(1.0f, 1.0f, 1.0f), q.origin, normalize(dir), 0, true};
        if (pc.max_bounces < 0) colour = colour + p.light * p.colour;  // trace_ray's loop does not run
      }
    }
    // (lanes without a regular segment due enter as inactive rays, as query_bvh's tail lanes do)
    const bool seg = !done && p.bounce <= pc.max_bounces;
    const bool reg = seg && segment_regular(p.pos, p.dir);
    const f3 o = reg ? p.pos : mk(0.0f, 0.0f, 0.0f), d = reg ? p.dir : mk(0.0f, 0.0f, 1.0f);
    Closest c{kFltMax, 0, 0u, 0u};
    Diag dg;
    world_hit_bounce_bvh<false>(sc, P, BvhGlobal{P.bvh_nodes, P.bvh_prims}, reg, o, d, tests, c, dg);
    if (seg && !reg) {
      c = world_hit_scan_from(sc, pc.num_spheres, pc.num_meshes, p.pos, p.dir, kFltMax, tests);
      ++scan;
    }
    if (seg) {
      ++segs;
      const bool ended = shade_step(sc, pc, p, c, state);
      ++p.bounce;
      if (ended || p.bounce > pc.max_bounces) {
        colour = colour + p.light * p.colour;
        p.bounce = pc.max_bounces + 1;
      }
    }
  }
  if (live) {
    colour = div3(colour, (float)pc.num_samples);
    Q.out[i] = make_float4(colour.x, colour.y, colour.z, 1.0f);
  }
  radiance_counts(Q.stats, scan, segs, tests);
}

// PAIRS: LDS carved exactly as query_pairs carves it; persistent workgroups.  A lane holds one query at a time
// (its index, the colour so far, the sample count, the path) and reads its record again at each sample's
// start.  Each trip of a wave: lanes whose query is complete store it; the idle lanes draw the next indices
// from Q.next -- one atomicAdd by the first idle lane for all of them, handed out in lane order -- until the
// counter has passed n (then `dry`, wave-uniform: no further atomics); lanes between paths start their next
// sample; lanes that owe a direction compute it (shade_dir); ALL 64 lanes enter the traversal, those without a
// regular segment due as inactive rays; irregular segments take the scan; every lane with a segment shades
// its hit (shade_hit).  Q.next never exceeds n + 64 x the grid's waves (a wave overshoots once), and a launch
// has n <= 2^31 (launch_radiance), so it does not wrap.
template <bool NodeR, bool Stats>
__global__ __launch_bounds__(1024) void radiance_pairs(TraceParams P, RadianceArgs Q) {
  const uint32_t nn = P.bvh_wq_n_nodes;
  float4* nodes = lds_tris;
  for (uint32_t k = threadIdx.x; k < 3 * nn; k += 1024) nodes[k] = P.bvh_wq_nodes[k];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  char* base = reinterpret_cast<char*>(nodes + 3 * nn) + (size_t)wave * (512 + 4 * (P.wq_ncap + P.wq_tcap));
  const WqLds wq{nodes, reinterpret_cast<unsigned long long*>(base), reinterpret_cast<uint32_t*>(base + 512),
                 reinterpret_cast<uint32_t*>(base + 512) + P.wq_ncap, P.wq_ncap, false};
  __syncthreads();
  const hrt_push_constants& pc = P.pc;
  uint32_t scan = 0, segs = 0, tests = 0;
  uint32_t qi = 0, state = 0;
  bool have = false, dry = false;
  f3 colour = mk(0.0f, 0.0f, 0.0f);
  int sample = 0;
  Path p{mk(0.0f, 0.0f, 0.0f), mk(1.0f, 1.0f, 1.0f), mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 1.0f), 0, true};
  p.bounce = pc.max_bounces + 1;  // no path under way
  Pending<true> pd;  // set only in a lane that then has a segment due, cleared by the next trip's shade_dir
  for (;;) {
    // (a loop: with num_samples <= 0 a query just drawn is complete at once and must still be stored)
    for (;;) {
      if (have && p.bounce > pc.max_bounces && sample >= pc.num_samples) {
        const f3 r = div3(colour, (float)pc.num_samples);
        Q.out[qi] = make_float4(r.x, r.y, r.z, 1.0f);
        have = false;
      }
      const unsigned long long nb = __ballot(!have);
      if (dry || !nb) break;
      const uint32_t cnt = (uint32_t)__popcll(nb), first = (uint32_t)__ffsll((long long)nb) - 1u;
      uint32_t got = 0;
      if (lane == first) got = atomicAdd(Q.next, cnt);
      const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)got, (int)first);
      dry = at >= Q.n || Q.n - at <= cnt;
      const uint32_t idx = at + lanes_below(nb);
      if (!have && idx < Q.n) {
        have = true;
        qi = idx;
        state = fbits(Q.queries[2 * (size_t)idx].w);
        colour = mk(0.0f, 0.0f, 0.0f);
        sample = 0;
      }
    }
    if (!__any(have)) break;
    if (have && p.bounce > pc.max_bounces) {  // (sample < num_samples: the query is not complete)
      ++sample;
      const RadianceRecord q = radiance_record(Q, qi);
      // the matrix and jitter read at the sample's start (kargs): not held in SGPRs across the loop
      const f3 dir = get_ray_dir(kargs()->pc, q.centre, state);
      p = Path{mk(0.0f, 0.0f, 0.0f), mk(1.0f, 1.0f, 1.0f), q.origin, normalize_fl(dir), 0, true};
      if (pc.max_bounces < 0) colour = colour + p.light * p.colour;  // trace_ray's loop does not run
    }
    const bool seg = have && p.bounce <= pc.max_bounces;
    if (__any(seg)) {
      if (seg && pd.id != 0u) shade_dir(kscene(), p, state, pd);
      const bool reg = seg && segment_regular(p.pos, p.dir);
      const f3 o = reg ? p.pos : mk(0.0f, 0.0f, 0.0f), d = reg ? p.dir : mk(0.0f, 0.0f, 1.0f);
      Closest c{kFltMax, 0, 0u, 0u};
      Diag dg;
      world_hit_bounce_wq<false, NodeR>(kscene(), P, wq, reg, o, d, tests, c, dg);
      if (seg && !reg) {
        const Scene sc = kscene();
        c = world_hit_scan_from(sc, pc.num_spheres, pc.num_meshes, p.pos, p.dir, kFltMax, tests);
        ++scan;
      }
      if (seg) {
        ++segs;
        const bool ended = shade_hit(kscene(), pc, p, c, state, p.bounce >= pc.max_bounces, pd);
        ++p.bounce;
        if (ended || p.bounce > pc.max_bounces) {
          colour = colour + p.light * p.colour;
          p.bounce = pc.max_bounces + 1;
        }
      }
      // a segment adds fewer than 2^26 tests (a hierarchy exists): flushed long before a lane's count wraps
      if (Stats && __any(tests >= 0x80000000u)) {
        radiance_counts(Q.stats, scan, segs, tests);
        scan = segs = tests = 0;
      }
    }
  }
  if (Stats) radiance_counts(Q.stats, scan, segs, tests);
}

hipError_t launch_radiance(const TraceParams& p0, const RadianceArgs& q, const QueryPlan& plan, hipStream_t stream) {
  if (q.n == 0) return hipSuccess;
  if (q.n > 0x80000000u) return hipErrorInvalidValue;
  const uint32_t blocks = (q.n + 255u) / 256u;
  switch (plan.method) {
    case HRT_QUERY_SCAN:
      radiance_scan<<<blocks, 256, 0, stream>>>(p0, q);
      break;
    case HRT_QUERY_BVH:
      radiance_bvh<<<blocks, 256, 0, stream>>>(p0, q);
      break;
    case HRT_QUERY_PAIRS: {
      if (plan.lds_bytes == 0 || !q.next) return hipErrorInvalidValue;
      TraceParams p = p0;
      p.wq_ncap = plan.wq_ncap;
      p.wq_tcap = plan.wq_tcap;
      // (their dynamic-LDS limit: ensure_kernel_attributes)
      void (*kernel)(TraceParams, RadianceArgs) =
          p.bvh_node_r ? (q.stats ? radiance_pairs<true, true> : radiance_pairs<true, false>)
                       : (q.stats ? radiance_pairs<false, true> : radiance_pairs<false, false>);
      if (hipError_t e = hipMemsetAsync(q.next, 0, sizeof(uint32_t), stream); e != hipSuccess) return e;
      const uint32_t groups = std::min((q.n + 1023u) / 1024u, std::max(1u, p.num_cus));
      kernel<<<groups, 1024, plan.lds_bytes, stream>>>(p, q);
      break;
    }
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ---- the first-hit pass: every pixel's un-jittered primary ray from the tile lists -----------
// hrt_intersect_primary's bytes for the whole image (S11), answered the way the frame kernels answer primary
// segments: one wave per 8x8 tile (tile_lists' lane-to-pixel map) builds the tile's list and tests only the
// listed records.  The lists are built for jitter reach 0 (the host passes pc.jitter_size = 0): the direction
// here is normalize(M c) of the pixel's own centre c, so each pixel's box is that one point (the soundness
// paragraph above refine_tile_list covers the S4 rounding).  A tile whose list is not usable -- build_tile_list
// says not ok (more than 32 meshes, more than 64 survivors, a cap wider than c_lo > 0.5, a corner that is not
// finite), or the scene has more meshes than world_hit_tile's octant word holds (8) -- takes world_hit_bundle,
// the per-wave cull of the same camera records; irregular lanes (query_ray's rule) take the literal scan as in
// query_finish.  No LDS, no persistent scheduling.  Count: the statistics of FirstHitsArgs (else no such code).
template <bool Count>
__global__ __launch_bounds__(256) void first_hits_tiles(TraceParams P, FirstHitsArgs A) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t W = P.pc.width, H = P.pc.height;
  const uint32_t tiles_x = (W + 7) / 8, tiles = tiles_x * ((H + 7) / 8);
  const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= tiles) return;  // wave-uniform
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const uint32_t x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
  const bool active = x < W && y < H;
  // the pass as a primary query of the whole image: ray i = pixel i (an inactive lane: past the end)
  const QueryArgs Q{nullptr, A.hits, Count ? A.stats : nullptr, W * H, 0u, 0u, 0u, W};
  const uint32_t i = active ? x + y * W : Q.n;
  f3 centre = mk(0.0f, 0.0f, 0.0f);
  if (active) {
    const float4 rc = P.rays[i];
    centre = mk(rc.x, rc.y, rc.z);
  }
  const QueryRay r = query_ray<true>(P, Q, i);
  const bool prim = r.live && r.finite;
  const f3 o = prim ? r.o : mk(0.0f, 0.0f, 0.0f), d = prim ? r.d : mk(0.0f, 0.0f, 1.0f);
  const TileList tl = build_tile_list(P, active, centre, nullptr);
  const bool listed = tl.ok && P.pc.num_meshes <= 8;
  const Scene sc{P.rays, P.spheres, P.tris, P.meshes, P.tri_nhat};
  uint32_t tests = 0, tested = 0;
  Closest c{kFltMax, 0, 0u, 0u};
  if (listed) {
    tested = world_hit_tile(sc, P, tl, prim, o, d, tests, c);
  } else if (__any(prim)) {
    Diag dg;
    world_hit_bundle<false>(sc, P, prim, o, d, tests, c, dg);
  }
  query_finish(sc, P, r, prim, c, tests);
  query_store(sc, Q, i, r, c, tests);
  if (Count && lane == 0) {
    atomicAdd(&A.stats[listed ? 2 : 4], 1ull);
    if (listed && tl.n == 0 && P.pc.num_spheres == 0) atomicAdd(&A.stats[3], 1ull);
    if (tested) atomicAdd(&A.stats[5], (unsigned long long)tested);
  }
}

hipError_t launch_first_hits_tiles(const TraceParams& p, const FirstHitsArgs& a, bool lists_ready, hipStream_t stream) {
  const uint32_t tiles = ((p.pc.width + 7) / 8) * ((p.pc.height + 7) / 8);
  if (tiles == 0) return hipSuccess;
  if (p.pc.num_meshes > 0 && !lists_ready) camera_lists<<<p.pc.num_meshes, 256, 0, stream>>>(p);
  if (a.stats)
    first_hits_tiles<true><<<(tiles + 3) / 4, 256, 0, stream>>>(p, a);
  else
    first_hits_tiles<false><<<(tiles + 3) / 4, 256, 0, stream>>>(p, a);
  return hipGetLastError();
}

}  // namespace hrt
