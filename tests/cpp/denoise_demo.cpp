// The denoise pass through include/hrt_app.hpp, the C++ mirror of the host surface: two 1-sample frames of a
// 48 x 32 view folded into the accumulator, the view's first hits kept on the device
// (RayTracePipeline::first_hits_into), then DiffusePipeline::denoised with that guide (RGBA32F) and without
// one (RGBA8), and RenderPassOverFrame::render_denoised into a device target.  tests/test_gpu_denoise.py runs
// the Python mirror on the same scene and compares the bytes.
//
//   denoise_demo <in.bin> <out.bin>
//
// Input (little-endian, written by the test from the Python scene): u32 spheres, per sphere 4 floats (centre,
// radius); u32 meshes, per mesh u32 vertices, u32 indices, the positions, the indices.  Every primitive is
// Lambertian grey; 1 sample, 4 bounces, environment light on.
// Output: u32 width, u32 height, the guided RGBA32F image, the colour-only RGBA8 image, the target's bytes
// (B8G8R8A8, pitch width * 4).  A library error prints its message and exits with 10 + the hrt_status.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hrt_app.hpp"

// the three HIP runtime calls the demo needs for its device buffers (hrt_app.hpp itself is HIP-free)
extern "C" int hipMalloc(void** ptr, size_t bytes);
extern "C" int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);
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
  void* guide = nullptr;
  void* target = nullptr;
  int rc = 0;
  try {
    const uint32_t w = 48, h = 32, npix = w * h;
    epq::Context ctx(w, h, -1, HRT_MODE_RGBA8);
    epq::RayTracePipeline pipe(ctx, {w, h}, s);
    epq::DiffusePipeline diffuse(ctx, {w, h});
    epq::RenderPassOverFrame pass(ctx);
    const epq::Camera camera{};
    for (uint32_t frame = 0; frame < 3; ++frame) {  // (frame 0 clears the accumulator)
      pipe.compute(camera, frame);
      diffuse.next_frame(frame, pipe.image());
    }
    if (hipMalloc(&guide, (size_t)npix * sizeof(hrt_hit)) != 0 || hipMalloc(&target, (size_t)npix * 4) != 0) return 5;
    pipe.first_hits_into(camera, static_cast<hrt_hit*>(guide));
    const std::vector<uint8_t> guided = diffuse.denoised(static_cast<const hrt_hit*>(guide), HRT_FMT_RGBA32F);
    const std::vector<uint8_t> plain = diffuse.denoised();
    const epq::PresentTarget pt{target, (uint64_t)npix * 4, w, h};
    ctx.present_wait(pass.render_denoised(diffuse.image(), pt, static_cast<const hrt_hit*>(guide)));
    std::vector<uint8_t> shown((size_t)npix * 4);
    if (hipMemcpy(shown.data(), target, shown.size(), 2 /* device to host */) != 0) return 5;
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(&w, 4, 1, f);
    std::fwrite(&h, 4, 1, f);
    std::fwrite(guided.data(), 1, guided.size(), f);
    std::fwrite(plain.data(), 1, plain.size(), f);
    std::fwrite(shown.data(), 1, shown.size(), f);
    std::fclose(f);
    std::printf("denoise_demo: %u x %u\n", w, h);
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "denoise_demo: %s\n", e.what());
    rc = 10 + (int)e.status;
  }
  (void)hipFree(guide);
  (void)hipFree(target);
  return rc;
}
