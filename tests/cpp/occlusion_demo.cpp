// Occlusion queries through include/hrt_app.hpp, the C++ mirror of the host surface: RayTracePipeline::visible
// of given point pairs, and RayTracePipeline::occluded of their segments' rays with t_max lifted to FLT_MAX.
// tests/test_gpu_occluded.py asks the Python mirror the same on the box scene and compares the answers.
//
//   occlusion_demo <in.bin> <out.bin>
//
// Input (little-endian, written by the test from the Python scene): u32 spheres, per sphere 4 floats (centre,
// radius); u32 meshes, per mesh u32 vertices, u32 indices, the positions, the indices; u32 pairs, the pairs'
// first points (3 floats each), then their second points.  Materials do not bear on occlusion: every
// primitive is Lambertian grey.  Output: u32 pairs, one byte per pair (visible), one byte per pair (occluded
// with t_max = FLT_MAX).  A library error prints its message and exits with 10 + the hrt_status.
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hrt_app.hpp"

template <class T>
static bool get(FILE* f, T* out, size_t n) {
  return std::fread(out, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  epq::RayTracerSettings s;
  s.num_samples = 1;
  s.max_bounces = 1;
  s.use_environment_lighting = true;
  const epq::LambertianMaterial grey{{0.5f, 0.5f, 0.5f}};
  uint32_t n_spheres = 0, n_meshes = 0, n = 0;
  if (!get(in, &n_spheres, 1) || n_spheres > (1u << 20)) return 4;
  for (uint32_t i = 0; i < n_spheres; ++i) {
    float v[4];
    if (!get(in, v, 4)) return 4;
    s.sphere_data.push_back(epq::Sphere{{v[0], v[1], v[2]}, v[3], grey});
  }
  if (!get(in, &n_meshes, 1) || n_meshes > 64) return 4;
  for (uint32_t m = 0; m < n_meshes; ++m) {
    uint32_t nv = 0, ni = 0;
    if (!get(in, &nv, 1) || !get(in, &ni, 1) || nv > (1u << 24) || ni > (1u << 26)) return 4;
    epq::Mesh mesh;
    mesh.positions.resize((size_t)nv * 3);
    mesh.indices.resize(ni);
    if (!get(in, mesh.positions.data(), mesh.positions.size()) || !get(in, mesh.indices.data(), ni)) return 4;
    s.mesh_data.push_back(epq::RayTracingMesh{mesh, grey});
  }
  if (!get(in, &n, 1) || n > (1u << 24)) return 4;
  std::vector<epq::Vec3> a(n), b(n);
  if (!get(in, a.data(), n) || !get(in, b.data(), n)) return 4;
  std::fclose(in);
  try {
    const uint32_t w = 16, h = 16;
    epq::Context ctx(w, h, -1, HRT_MODE_RGBA8);
    epq::RayTracePipeline pipe(ctx, {w, h}, s);
    const std::vector<bool> vis = pipe.visible(a, b);
    std::vector<hrt_ray_query> rays(n);
    for (uint32_t i = 0; i < n; ++i) {
      rays[i] = epq::RayTracePipeline::segment_ray(a[i], b[i]);
      rays[i].t_max = FLT_MAX;
    }
    const std::vector<bool> occ = pipe.occluded(rays);
    std::vector<uint8_t> out(2 * (size_t)n);
    uint32_t seen = 0;
    for (uint32_t i = 0; i < n; ++i) {
      out[i] = vis[i] ? 1 : 0;
      out[n + i] = occ[i] ? 1 : 0;
      seen += out[i];
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(&n, 4, 1, f);
    std::fwrite(out.data(), 1, out.size(), f);
    std::fclose(f);
    std::printf("occlusion_demo: %u of %u point pairs see each other\n", seen, n);
    return 0;
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "occlusion_demo: %s\n", e.what());
    return 10 + (int)e.status;
  }
}
