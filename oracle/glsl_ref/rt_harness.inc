// oracle/glsl_ref/rt_harness.inc -- C ABI around the translated path-trace shader (appended to the generated unit by
// translate.py; see glsl_shim.hpp).  This project's own code: it calls the shader's functions by name and holds none
// of their text.  Every batched entry runs n independent cases; `states` arrays are read and written back.
#include <cstring>
#include <thread>
#include <vector>

namespace R = glsl::raytracing;
using glsl::vec3;
using glsl::vec4;

// std430 sizes (raytracing.glsl:51-101, :135-153): the host uploads exactly these records
static_assert(sizeof(R::PushConstants) == 124, "push constants");
static_assert(sizeof(R::Sphere) == 64, "Sphere");
static_assert(sizeof(R::Triangle) == 64, "Triangle");
static_assert(sizeof(R::Mesh) == 80, "Mesh");
static_assert(sizeof(R::Ray) == 16, "Ray");
static_assert(sizeof(R::RayTracingMaterial) == 48, "RayTracingMaterial");
static_assert(sizeof(glsl::bool32) == 4 && sizeof(glsl::mat4) == 64, "shim");

namespace {

// the calling thread's copy of the shader's globals
void bind(const R::PushConstants* pc, const void* rays, const void* spheres, const void* tris, const void* meshes) {
  if (pc) R::push_constants = *pc;
  R::rays.data = static_cast<const R::Ray*>(rays);
  R::spheres.data = static_cast<const R::Sphere*>(spheres);
  R::triangles.data = static_cast<const R::Triangle*>(tris);
  R::meshes.data = static_cast<const R::Mesh*>(meshes);
  R::triangles.reads = 0;
}
inline vec3 ld3(const float* p) { return vec3(p[0], p[1], p[2]); }
inline void st3(float* p, vec3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
// a RayHit as 19 floats: normal, position, distance, material (colour, emission, settings)
inline void st_hit(float* p, const R::RayHit& h) {
  st3(p, h.hit_normal); st3(p + 3, h.hit_pos); p[6] = h.hit_dist;
  std::memcpy(p + 7, &h.hit_mat, 48);
}

// The sequenced restatement of raytracing.glsl:163-165 for the evaluation-order check: u1, then u2 into the z term,
// then u3 into the y term, one statement per operation.  `swapped` draws u3 before u2 instead (what a compiler that
// evaluates the second operand of `+` first computes).
vec3 ray_dir_sequenced(vec3 centre, glsl::uint& state, bool swapped) {
  const R::PushConstants& pc = R::push_constants;
  float u1 = R::scaleToRange01(R::hash(state));
  float angle = u1 * 2;
  angle = angle * M_PI;
  float first = R::scaleToRange01(R::hash(state));
  float second = R::scaleToRange01(R::hash(state));
  float u2 = swapped ? second : first, u3 = swapped ? first : second;
  float c = glsl::cos(angle);
  vec3 tz = c * vec3(0, 0, 1);
  tz = tz * pc.jitter_size;
  tz = tz * glsl::sqrt(u2);
  vec3 acc = centre + tz;
  float s = glsl::sin(angle);
  vec3 ty = s * vec3(0, 1, 0);
  ty = ty * pc.jitter_size;
  ty = ty * glsl::sqrt(u3);
  acc = acc + ty;
  vec3 world = glsl::mat3(pc.cam_alignment_mat) * acc;
  return glsl::normalize(world);
}

inline bool same3(vec3 a, vec3 b) { return std::memcmp(&a, &b, 12) == 0; }

}  // namespace

extern "C" {

// 0 when the compiler evaluated raytracing.glsl:164's two draws left to right on every probe state (and the probe
// can tell: the swapped order gives other bits on most of them); otherwise the number of states that disagree, or -1
// when the probe cannot tell the two orders apart.
int glr_selfcheck(void) {
  R::PushConstants pc;
  std::memset(&pc, 0, sizeof pc);
  const float m[16] = {0.36f, 0.48f, -0.8f, 0.0f, -0.8f, 0.6f, 0.0f, 0.0f, 0.48f, 0.64f, 0.6f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  std::memcpy(&pc.cam_alignment_mat, m, sizeof m);
  pc.jitter_size = 0.37f;
  bind(&pc, nullptr, nullptr, nullptr, nullptr);
  int bad = 0, told_apart = 0;
  const int n = 4096;
  for (int k = 0; k < n; k++) {
    glsl::uint s0 = 0x9E3779B9u * glsl::uint(k) + 12345u, a = s0, b = s0, c = s0;
    vec3 centre(1.0f, 0.001f * float(k % 97) - 0.05f, 0.0007f * float(k % 89) - 0.03f);
    vec3 shader = R::get_ray_dir(centre, a);
    vec3 want = ray_dir_sequenced(centre, b, false);
    vec3 other = ray_dir_sequenced(centre, c, true);
    if (!same3(shader, want) || a != b) bad++;
    if (!same3(want, other)) told_apart++;
  }
  if (told_apart < n / 2) return -1;
  return bad;
}

// ---- frames ------------------------------------------------------------------------------------------------------
// The rows [y0, y1) of a frame.  rgba8 (H*W*4 bytes), rgba32f (H*W*4 floats: the vec4 given to imageStore, before
// quantisation) and tri_tests (reads of the triangle buffer) may each be null.  main() runs for x < width and
// y < height only: the shader's own bound (raytracing.glsl:359) is `>`, which lets one more column and row of
// invocations through to stores outside the image, which Vulkan drops -- the known harmless quirk, not exercised here.
void glr_trace_rows(const R::PushConstants* pc, const void* rays, const void* spheres, const void* tris,
                    const void* meshes, uint32_t y0, uint32_t y1, uint8_t* rgba8, float* rgba32f, uint64_t* tri_tests,
                    int nthreads) {
  if (y1 > pc->height) y1 = pc->height;
  if (nthreads <= 0) nthreads = int(std::thread::hardware_concurrency());
  if (nthreads > 16) nthreads = 16;
  if (nthreads < 1 || y1 <= y0 + 1) nthreads = 1;
  std::vector<uint64_t> reads(size_t(nthreads), 0);
  auto work = [&](int t) {
    bind(pc, rays, spheres, tris, meshes);
    R::img.texels = rgba8; R::img.stored = rgba32f; R::img.width = pc->width; R::img.height = pc->height;
    for (uint32_t y = y0 + uint32_t(t); y < y1; y += uint32_t(nthreads))
      for (uint32_t x = 0; x < pc->width; x++) {
        R::gl_GlobalInvocationID = glsl::uvec3{x, y, 0};
        R::shader_main();
      }
    reads[size_t(t)] = R::triangles.reads;
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < nthreads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  uint64_t sum = 0;
  for (uint64_t r : reads) sum += r;
  if (tri_tests) *tri_tests = sum;
}

// The listed pixels (xy[2k], xy[2k+1]) of one frame: out32f[4k..] the stored vec4, out8[4k..] its texel, tests[k] the
// pixel's own triangle-buffer reads (each may be null).
void glr_trace_pixels(const R::PushConstants* pc, const void* rays, const void* spheres, const void* tris,
                      const void* meshes, const uint32_t* xy, uint32_t n, float* out32f, uint8_t* out8, uint64_t* tests) {
  bind(pc, rays, spheres, tris, meshes);
  std::vector<uint8_t> t8(size_t(pc->width) * pc->height * 4);
  std::vector<float> t32(size_t(pc->width) * pc->height * 4);
  R::img.texels = t8.data(); R::img.stored = t32.data(); R::img.width = pc->width; R::img.height = pc->height;
  for (uint32_t k = 0; k < n; k++) {
    uint32_t x = xy[2 * k], y = xy[2 * k + 1];
    if (x >= pc->width || y >= pc->height) continue;
    uint64_t before = R::triangles.reads;
    R::gl_GlobalInvocationID = glsl::uvec3{x, y, 0};
    R::shader_main();
    size_t p = (size_t(y) * pc->width + x) * 4;
    if (out32f) std::memcpy(out32f + 4 * k, &t32[p], 16);
    if (out8) std::memcpy(out8 + 4 * k, &t8[p], 4);
    if (tests) tests[k] = R::triangles.reads - before;
  }
}

// ---- the shader's functions, n cases each ------------------------------------------------------------------------
void glr_hash(uint32_t n, uint32_t* states, uint32_t* out) {
  for (uint32_t k = 0; k < n; k++) out[k] = R::hash(states[k]);
}
void glr_scale01(uint32_t n, const uint32_t* in, float* out) {
  for (uint32_t k = 0; k < n; k++) out[k] = R::scaleToRange01(in[k]);
}
void glr_normal_dist(uint32_t n, uint32_t* states, float* out) {
  for (uint32_t k = 0; k < n; k++) out[k] = R::RandomValueNormalDistribution(states[k]);
}
void glr_point_on_sphere(uint32_t n, uint32_t* states, float* out) {
  for (uint32_t k = 0; k < n; k++) st3(out + 3 * k, R::RandomPointOnUnitSphere(states[k]));
}
void glr_point_on_hemisphere(uint32_t n, uint32_t* states, const float* normals, float* out) {
  for (uint32_t k = 0; k < n; k++) st3(out + 3 * k, R::RandomPointOnHemisphere(states[k], ld3(normals + 3 * k)));
}
void glr_get_ray_dir(uint32_t n, const R::PushConstants* pc, const float* centres, uint32_t* states, float* out) {
  bind(pc, nullptr, nullptr, nullptr, nullptr);
  for (uint32_t k = 0; k < n; k++) st3(out + 3 * k, R::get_ray_dir(ld3(centres + 3 * k), states[k]));
}
void glr_intersecting_sphere(uint32_t n, const R::Sphere* spheres, const float* o, const float* d, float* out) {
  for (uint32_t k = 0; k < n; k++) st_hit(out + 19 * k, R::intersecting_sphere(spheres[k], ld3(o + 3 * k), ld3(d + 3 * k)));
}
void glr_intersecting_aabb(uint32_t n, const float* mn, const float* mx, const float* o, const float* d, int32_t* out) {
  for (uint32_t k = 0; k < n; k++)
    out[k] = R::intersecting_aabb(ld3(mn + 3 * k), ld3(mx + 3 * k), ld3(o + 3 * k), ld3(d + 3 * k)) ? 1 : 0;
}
void glr_intersecting_tri(uint32_t n, const R::Triangle* tris, const float* o, const float* d, float* out) {
  for (uint32_t k = 0; k < n; k++) {
    vec4 r = R::intersecting_tri(tris[k], ld3(o + 3 * k), ld3(d + 3 * k));
    std::memcpy(out + 4 * k, &r, 16);
  }
}
void glr_intersecting_mesh(uint32_t n, const void* tris, const R::Mesh* mesh, const float* o, const float* d, float* out,
                           uint64_t* tri_tests) {
  bind(nullptr, nullptr, nullptr, tris, nullptr);
  for (uint32_t k = 0; k < n; k++) st_hit(out + 19 * k, R::intersecting_mesh(*mesh, ld3(o + 3 * k), ld3(d + 3 * k)));
  if (tri_tests) *tri_tests = R::triangles.reads;
}
void glr_world_hit(uint32_t n, const R::PushConstants* pc, const void* spheres, const void* tris, const void* meshes,
                   const float* o, const float* d, float* out, uint64_t* tri_tests) {
  bind(pc, nullptr, spheres, tris, meshes);
  for (uint32_t k = 0; k < n; k++) st_hit(out + 19 * k, R::world_hit(ld3(o + 3 * k), ld3(d + 3 * k)));
  if (tri_tests) *tri_tests = R::triangles.reads;
}
void glr_environment_light(uint32_t n, const R::PushConstants* pc, const float* d, float* out) {
  bind(pc, nullptr, nullptr, nullptr, nullptr);
  for (uint32_t k = 0; k < n; k++) st3(out + 3 * k, R::environment_light(ld3(d + 3 * k)));
}
void glr_adjust_dir(uint32_t n, const float* d, const float* normals, const R::RayTracingMaterial* mats,
                    const int32_t* specular, uint32_t* states, float* out) {
  for (uint32_t k = 0; k < n; k++)
    st3(out + 3 * k, R::adjust_dir(ld3(d + 3 * k), ld3(normals + 3 * k), mats[k], specular[k] != 0, states[k]));
}
void glr_trace_ray(uint32_t n, const R::PushConstants* pc, const void* spheres, const void* tris, const void* meshes,
                   const float* o, const float* d, uint32_t* states, float* out, uint64_t* tri_tests) {
  bind(pc, nullptr, spheres, tris, meshes);
  for (uint32_t k = 0; k < n; k++) st3(out + 3 * k, R::trace_ray(ld3(o + 3 * k), ld3(d + 3 * k), states[k]));
  if (tri_tests) *tri_tests = R::triangles.reads;
}

// ---- the shim's own builtins, for tests of the shim against float64 ----------------------------------------------
// op: 0 dot (out[1]), 1 cross, 2 normalize (a only), 3 reflect(a, b), 4 mix(a, b, t[k]) (out[3])
void glr_shim_op(int op, uint32_t n, const float* a, const float* b, const float* t, float* out) {
  for (uint32_t k = 0; k < n; k++) {
    vec3 x = ld3(a + 3 * k), y = b ? ld3(b + 3 * k) : vec3(0.0f);
    switch (op) {
      case 0: out[k] = glsl::dot(x, y); break;
      case 1: st3(out + 3 * k, glsl::cross(x, y)); break;
      case 2: st3(out + 3 * k, glsl::normalize(x)); break;
      case 3: st3(out + 3 * k, glsl::reflect(x, y)); break;
      default: st3(out + 3 * k, glsl::mix(x, y, t[k])); break;
    }
  }
}
// imageStore of (v, v, v, v) into a one-texel rgba8 image, then imageLoad: bytes[k] and loaded[k] of the x channel
void glr_shim_store_load(uint32_t n, const float* v, uint8_t* bytes, float* loaded) {
  uint8_t texel[4];
  glsl::image2D im;
  im.texels = texel; im.width = 1; im.height = 1;
  for (uint32_t k = 0; k < n; k++) {
    glsl::imageStore(im, glsl::ivec2(0, 0), vec4(v[k]));
    bytes[k] = texel[0];
    loaded[k] = glsl::imageLoad(im, glsl::ivec2(0, 0)).x;
  }
}

}  // extern "C"
