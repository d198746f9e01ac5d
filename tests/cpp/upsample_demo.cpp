// Guided upsampling through include/hrt_app.hpp, the C++ mirror of the host surface: three 1-sample frames of a
// 24 x 16 view accumulated on one context, the same view's first hits at 24 x 16 (RayTracePipeline::first_hits_into)
// and at 48 x 32 on a second context of the same scene (RayTracePipeline::first_hits_enqueue, not waited for), then
// Context::upsample to 48 x 32 (RGBA32F, footprint 4) and RenderPassOverFrame::render_upsampled into a device target
// (the default footprint), ordered after the second context's stream by Context::order_after.
// tests/test_gpu_upsample.py runs the Python mirror on the same scene and compares the bytes.
//
//   upsample_demo <in.bin> <out.bin>
//
// Input (little-endian, written by the test from the Python scene): u32 spheres, per sphere 4 floats (centre,
// radius); u32 meshes, per mesh u32 vertices, u32 indices, the positions, the indices.  Every primitive is
// Lambertian grey; 1 sample, 4 bounces, environment light on, RGBA32F.
// Output: u32 width, u32 height of the target, the upsampled image (RGBA32F) and the target's bytes
// (width x height x 4).  A library error prints its message and exits with 10 + the hrt_status.
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
    const uint32_t ws = 24, hs = 16, w = 48, h = 32, npix = w * h;
    epq::Context low(ws, hs, -1, HRT_MODE_RGBA32F), high(w, h, -1, HRT_MODE_RGBA32F);
    epq::RayTracePipeline pipe(low, {ws, hs}, s), guide_pipe(high, {w, h}, s);
    epq::DiffusePipeline diffuse(low, {ws, hs});
    const epq::Camera cam{};
    for (uint32_t frame = 0; frame < 3; ++frame) {
      pipe.compute(cam, frame);
      diffuse.next_frame(frame, pipe.image());
    }
    if (hipMalloc(&hits[0], (size_t)ws * hs * sizeof(hrt_hit)) != 0) return 5;
    if (hipMalloc(&hits[1], (size_t)npix * sizeof(hrt_hit)) != 0) return 5;
    if (hipMalloc(&target, (size_t)npix * 4) != 0) return 5;
    pipe.first_hits_into(cam, static_cast<hrt_hit*>(hits[0]));
    guide_pipe.first_hits_enqueue(cam, static_cast<hrt_hit*>(hits[1]));
    const hrt_hit* lo = static_cast<const hrt_hit*>(hits[0]);
    const hrt_hit* hi = static_cast<const hrt_hit*>(hits[1]);
    epq::RenderPassOverFrame pass(low);
    const epq::PresentTarget pt{target, (uint64_t)npix * 4, w, h};
    low.present_wait(pass.render_upsampled(diffuse.image(), pt, lo, hi, &high));
    hrt_upsample_info info = epq::Context::upsample_defaults(w, h);
    info.footprint = 4;
    const std::vector<uint8_t> up = low.upsample(info, lo, hi, HRT_FMT_RGBA32F);
    std::vector<uint8_t> shown((size_t)npix * 4);
    if (hipMemcpy(shown.data(), target, shown.size(), 2 /* device to host */) != 0) return 5;
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(&w, 4, 1, f);
    std::fwrite(&h, 4, 1, f);
    std::fwrite(up.data(), 1, up.size(), f);
    std::fwrite(shown.data(), 1, shown.size(), f);
    std::fclose(f);
    std::printf("upsample_demo: %u x %u -> %u x %u\n", ws, hs, w, h);
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "upsample_demo: %s\n", e.what());
    rc = 10 + (int)e.status;
  }
  (void)hipFree(hits[0]);
  (void)hipFree(hits[1]);
  (void)hipFree(target);
  return rc;
}
