// Object motion in the temporal history through include/hrt_app.hpp, the C++ mirror of the host surface: three
// 1-sample frames of a 48 x 32 view folded with per-pixel counts and moments, the first hits kept on the device, then
// every sphere of the scene slid by (0, 0.05, 0.3) -- a second RayTracePipeline on the same context, that is a second
// hrt_set_scene -- the new first hits, Context::reproject_motion_moments with epq::motion_between of the two poses
// for every sphere, and one frame of the new state folded in.  tests/test_gpu_motion.py runs the Python mirror on
// the same scene and compares the bytes.
//
//   motion_demo <in.bin> <out.bin>
//
// Input: as history_demo's.  Every primitive is Lambertian grey; 1 sample, 4 bounces, environment light on, RGBA32F.
// Output: u32 width, u32 height, then the count image, the moments image and the RGBA32F accumulator after the last
// fold.  A library error prints its message and exits with 10 + the hrt_status.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hrt_app.hpp"

// the two HIP runtime calls the demo needs for its device buffers (hrt_app.hpp itself is HIP-free)
extern "C" int hipMalloc(void** ptr, size_t bytes);
extern "C" int hipFree(void* ptr);

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
  if (!get(in, &n_spheres, 1) || n_spheres > (1u << 16)) return 4;
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
  const float shift[3] = {0.0f, 0.05f, 0.3f};
  epq::RayTracerSettings moved = s;
  for (auto& sp : moved.sphere_data)
    for (int c = 0; c < 3; ++c) sp.centre[c] = sp.centre[c] + shift[c];
  void* hits[2] = {nullptr, nullptr};
  int rc = 0;
  try {
    const uint32_t w = 48, h = 32, npix = w * h;
    epq::Context ctx(w, h, -1, HRT_MODE_RGBA32F);
    epq::DiffusePipeline diffuse(ctx, {w, h});
    epq::Camera cam{};  // the box preset's
    cam.position = {1.5f, 1.0f, 0.0f};
    cam.direction = {-1.0f, 0.0f, 0.0f};
    const hrt_view view = epq::view_of(cam, {w, h}, s);
    for (void*& p : hits)
      if (hipMalloc(&p, (size_t)npix * sizeof(hrt_hit)) != 0) return 5;
    {
      epq::RayTracePipeline pipe(ctx, {w, h}, s);
      for (uint32_t frame = 0; frame < 3; ++frame) {
        pipe.compute(cam, frame);
        diffuse.next_frame_history(pipe.image(), 32, true);
      }
      pipe.first_hits_into(cam, static_cast<hrt_hit*>(hits[0]));
    }
    epq::RayTracePipeline pipe(ctx, {w, h}, moved);  // hrt_set_scene: the accumulator, the counts and the moments stay
    pipe.first_hits_into(cam, static_cast<hrt_hit*>(hits[1]));
    const std::array<float, 12> before{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const std::array<float, 12> after{1, 0, 0, 0, 1, 0, 0, 0, 1, shift[0], shift[1], shift[2]};
    const std::vector<hrt_motion> spheres(n_spheres, epq::motion_between(before, after));
    ctx.reproject_motion_moments(spheres, {}, view, static_cast<const hrt_hit*>(hits[0]), view,
                                 static_cast<const hrt_hit*>(hits[1]));
    pipe.compute(cam, 3);
    diffuse.next_frame_history(pipe.image(), 32, true);
    const std::vector<uint32_t> counts = ctx.read_history();
    const std::vector<float> moments = ctx.read_moments();
    const std::vector<uint8_t> acc = ctx.read(HRT_IMG_ACCUM, HRT_FMT_RGBA32F);
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(&w, 4, 1, f);
    std::fwrite(&h, 4, 1, f);
    std::fwrite(counts.data(), 4, counts.size(), f);
    std::fwrite(moments.data(), 4, moments.size(), f);
    std::fwrite(acc.data(), 1, acc.size(), f);
    std::fclose(f);
    std::printf("motion_demo: %u x %u\n", w, h);
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "motion_demo: %s\n", e.what());
    rc = 10 + (int)e.status;
  }
  (void)hipFree(hits[0]);
  (void)hipFree(hits[1]);
  return rc;
}
