// The variance-guided denoise through include/hrt_app.hpp, the C++ mirror of the host surface: three 1-sample
// frames of a 48 x 32 view folded with per-pixel counts and luminance moments
// (DiffusePipeline::next_frame_history with moments), a camera move, the first hits of both views kept on the
// device (RayTracePipeline::first_hits_into), Context::reproject_moments with the default thresholds, two frames
// of the new view folded in, then DiffusePipeline::variance_denoised guided by the new view's first hits (RGBA32F,
// with the filtered variance) and RenderPassOverFrame::render_variance_denoised into a device target.
// tests/test_gpu_variance.py runs the Python mirror on the same scene and compares the bytes.
//
//   variance_demo <in.bin> <out.bin>
//
// Input (little-endian, written by the test from the Python scene): u32 spheres, per sphere 4 floats (centre,
// radius); u32 meshes, per mesh u32 vertices, u32 indices, the positions, the indices.  Every primitive is
// Lambertian grey; 1 sample, 4 bounces, environment light on, RGBA32F.
// Output: u32 width, u32 height, the moments image after the last fold (2 floats per pixel), the filtered image
// (RGBA32F), the filtered variance (1 float per pixel) and the target's bytes (width x height x 4).  A library
// error prints its message and exits with 10 + the hrt_status.
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
  void* hits[2] = {nullptr, nullptr};
  void* target = nullptr;
  int rc = 0;
  try {
    const uint32_t w = 48, h = 32, npix = w * h;
    epq::Context ctx(w, h, -1, HRT_MODE_RGBA32F);
    epq::RayTracePipeline pipe(ctx, {w, h}, s);
    epq::DiffusePipeline diffuse(ctx, {w, h});
    const epq::Camera before{};
    epq::Camera after{};
    after.position = {0.05f, 0.02f, -0.03f};
    after.direction = {1.0f, 0.03f, 0.08f};
    for (uint32_t frame = 0; frame < 3; ++frame) {
      pipe.compute(before, frame);
      diffuse.next_frame_history(pipe.image(), 32, true);
    }
    for (void*& p : hits)
      if (hipMalloc(&p, (size_t)npix * sizeof(hrt_hit)) != 0) return 5;
    if (hipMalloc(&target, (size_t)npix * 4) != 0) return 5;
    pipe.first_hits_into(before, static_cast<hrt_hit*>(hits[0]));
    pipe.first_hits_into(after, static_cast<hrt_hit*>(hits[1]));
    const hrt_hit* guide = static_cast<const hrt_hit*>(hits[1]);
    ctx.reproject_moments(epq::view_of(before, {w, h}, s), static_cast<const hrt_hit*>(hits[0]),
                          epq::view_of(after, {w, h}, s), guide);
    for (uint32_t frame = 3; frame < 5; ++frame) {
      pipe.compute(after, frame);
      diffuse.next_frame_history(pipe.image(), 32, true);
    }
    const std::vector<float> moments = ctx.read_moments();
    std::vector<float> variance;
    const std::vector<uint8_t> filtered = diffuse.variance_denoised(guide, HRT_FMT_RGBA32F, nullptr, &variance);
    epq::RenderPassOverFrame pass(ctx);
    const epq::PresentTarget pt{target, (uint64_t)npix * 4, w, h};
    ctx.present_wait(pass.render_variance_denoised(diffuse.image(), pt, guide));
    std::vector<uint8_t> shown((size_t)npix * 4);
    if (hipMemcpy(shown.data(), target, shown.size(), 2 /* device to host */) != 0) return 5;
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(&w, 4, 1, f);
    std::fwrite(&h, 4, 1, f);
    std::fwrite(moments.data(), 4, moments.size(), f);
    std::fwrite(filtered.data(), 1, filtered.size(), f);
    std::fwrite(variance.data(), 4, variance.size(), f);
    std::fwrite(shown.data(), 1, shown.size(), f);
    std::fclose(f);
    std::printf("variance_demo: %u x %u\n", w, h);
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "variance_demo: %s\n", e.what());
    rc = 10 + (int)e.status;
  }
  (void)hipFree(hits[0]);
  (void)hipFree(hits[1]);
  (void)hipFree(target);
  return rc;
}
