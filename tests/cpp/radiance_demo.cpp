// Radiance queries through include/hrt_app.hpp, the C++ mirror of the host surface: RayTracePipeline::radiance
// of given query records under the default camera's push block, and RayTracePipeline::radiance_pixels of every
// pixel of frame 3 of a 16 x 16 view.  tests/test_gpu_radiance.py asks the Python mirror the same on the box
// scene's geometry and compares the bytes.
//
//   radiance_demo <in.bin> <out.bin>
//
// Input (little-endian, written by the test from the Python scene): u32 spheres, per sphere 4 floats (centre,
// radius); u32 meshes, per mesh u32 vertices, u32 indices, the positions, the indices; u32 queries, the
// hrt_radiance_query records.  Every primitive is Lambertian grey; 3 samples, 4 bounces, environment light on.
// Output: u32 queries, u32 pixels, 4 floats per query, 4 floats per pixel.  A library error prints its message
// and exits with 10 + the hrt_status.
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
  s.num_samples = 3;
  s.max_bounces = 4;
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
  std::vector<hrt_radiance_query> queries(n);
  if (!get(in, queries.data(), n)) return 4;
  std::fclose(in);
  try {
    const uint32_t w = 16, h = 16, npix = w * h;
    epq::Context ctx(w, h, -1, HRT_MODE_RGBA8);
    epq::RayTracePipeline pipe(ctx, {w, h}, s);
    const epq::Camera camera{};
    const std::vector<std::array<float, 4>> asked = pipe.radiance(queries, camera);
    std::vector<uint32_t> xs(npix), ys(npix);
    for (uint32_t i = 0; i < npix; ++i) {
      xs[i] = i % w;
      ys[i] = i / w;
    }
    const std::vector<std::array<float, 4>> pixels = pipe.radiance_pixels(camera, xs, ys, 3u);
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(&n, 4, 1, f);
    std::fwrite(&npix, 4, 1, f);
    std::fwrite(asked.data(), 16, asked.size(), f);
    std::fwrite(pixels.data(), 16, pixels.size(), f);
    std::fclose(f);
    std::printf("radiance_demo: %u queries, %u pixels\n", n, npix);
    return 0;
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "radiance_demo: %s\n", e.what());
    return 10 + (int)e.status;
  }
}
