// Temporal upsampling through include/hrt_app.hpp, the C++ mirror of the host surface: five 1-sample frames of a
// 24 x 16 view, each traced on a grid shifted by epq::history_phase of the frame (Context::set_ray_grid) and folded
// into the history of a 48 x 32 context with moments (Context::accumulate_history_from), nothing waited for in
// between -- after the four phases every pixel of the large image has had a sample of its own.
// tests/test_gpu_resolve.py runs the Python mirror on the same scene and compares the bytes.
//
//   resolve_demo <in.bin> <out.bin>
//
// Input: as upsample_demo's (spheres, then meshes; every primitive Lambertian grey; 1 sample, 4 bounces, environment
// light on, RGBA32F).
// Output: u32 width, u32 height of the large image, its accumulator (RGBA32F), its counts (u32) and its moments
// (two floats per pixel).  A library error prints its message and exits with 10 + the hrt_status.
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
  s.max_bounces = 4;
  s.use_environment_lighting = true;
  const epq::LambertianMaterial grey{{0.5f, 0.5f, 0.5f}};
  uint32_t n_spheres = 0, n_meshes = 0;
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
  std::fclose(in);
  int rc = 0;
  try {
    const uint32_t ws = 24, hs = 16, w = 48, h = 32;
    epq::Context low(ws, hs, -1, HRT_MODE_RGBA32F), high(w, h, -1, HRT_MODE_RGBA32F);
    epq::RayTracePipeline pipe(low, {ws, hs}, s);
    const epq::Camera cam{};
    float first[3], dx[3], dy[3];
    (void)hrt_host_ray_grid(ws, hs, s.camera_focal_length, s.viewport_height, s.up.data(), first, dx, dy, nullptr);
    for (uint32_t frame = 0; frame < 5; ++frame) {
      const std::array<float, 2> phase = epq::history_phase({ws, hs}, {w, h}, frame);
      low.set_ray_grid(first, dx, dy, phase);
      pipe.compute(cam, frame);
      hrt_resolve_info info = epq::Context::resolve_defaults(phase);
      info.flags |= HRT_RESOLVE_MOMENTS;
      high.accumulate_history_from(low, info);
    }
    const std::vector<uint8_t> acc = high.read(HRT_IMG_ACCUM, HRT_FMT_RGBA32F);
    const std::vector<uint32_t> cnt = high.read_history();
    const std::vector<float> mom = high.read_moments();
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(&w, 4, 1, f);
    std::fwrite(&h, 4, 1, f);
    std::fwrite(acc.data(), 1, acc.size(), f);
    std::fwrite(cnt.data(), 4, cnt.size(), f);
    std::fwrite(mom.data(), 4, mom.size(), f);
    std::fclose(f);
    std::printf("resolve_demo: %u x %u -> %u x %u\n", ws, hs, w, h);
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "resolve_demo: %s\n", e.what());
    rc = 10 + (int)e.status;
  }
  return rc;
}
