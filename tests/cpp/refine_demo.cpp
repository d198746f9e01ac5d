// Adaptive refinement through include/hrt_app.hpp, the C++ mirror of the host surface: four 1-sample frames of a
// 48 x 32 view folded with per-pixel counts and luminance moments (DiffusePipeline::next_frame_history with moments),
// the view's first hits enqueued on the device (RayTracePipeline::first_hits_enqueue), Context::refine_select under
// the default rule guided by them, then DiffusePipeline::refine_until for three passes with the frames 4, 5, 6.
// tests/test_gpu_refine.py runs the Python mirror on the same scene and compares the bytes.
//
//   refine_demo <in.bin> <out.bin>
//
// Input (little-endian, written by the test from the Python scene): u32 spheres, per sphere 4 floats (centre,
// radius); u32 meshes, per mesh u32 vertices, u32 indices, the positions, the indices.  Every primitive is
// Lambertian grey; 1 sample, 4 bounces, environment light on, RGBA32F.
// Output: four u64 -- width, height, the pixels the selection marked, the pixel-frames the three passes traced --
// then the selection's mask words, the count image and the accumulator (RGBA32F) after the passes.  A library error
// prints its message and exits with 10 + the hrt_status.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hrt_app.hpp"

// the HIP runtime calls the demo needs for its device buffer (hrt_app.hpp itself is HIP-free)
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
  void* hits = nullptr;
  int rc = 0;
  try {
    const uint32_t w = 48, h = 32, npix = w * h;
    epq::Context ctx(w, h, -1, HRT_MODE_RGBA32F);
    epq::RayTracePipeline pipe(ctx, {w, h}, s);
    epq::DiffusePipeline diffuse(ctx, {w, h});
    epq::Camera cam{};  // outside the box, looking at its lit outer walls: noisy walls, a settled sky
    cam.position = {3.0f, 1.5f, 2.0f};
    cam.direction = {-0.8f, -0.3f, -0.6f};
    for (uint32_t frame = 0; frame < 4; ++frame) {
      pipe.compute(cam, frame);
      diffuse.next_frame_history(pipe.image(), HRT_HISTORY_MAX, true);
    }
    if (hipMalloc(&hits, (size_t)npix * sizeof(hrt_hit)) != 0) return 5;
    const hrt_hit* guide = static_cast<const hrt_hit*>(hits);
    pipe.first_hits_enqueue(cam, static_cast<hrt_hit*>(hits));
    uint64_t selected = 0;
    const std::vector<uint32_t> mask = ctx.refine_select(epq::Context::refine_defaults(), guide, &selected);
    const epq::Context::RefineResult res = diffuse.refine_until(pipe, cam, 4, 3, HRT_HISTORY_MAX, guide);
    if (res.passes != 3 || res.settled) return 6;
    const std::vector<uint32_t> counts = ctx.read_history();
    const std::vector<uint8_t> acc = ctx.read(HRT_IMG_ACCUM, HRT_FMT_RGBA32F);
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    const uint64_t head[4] = {w, h, selected, res.pixel_frames};
    std::fwrite(head, 8, 4, f);
    std::fwrite(mask.data(), 4, mask.size(), f);
    std::fwrite(counts.data(), 4, counts.size(), f);
    std::fwrite(acc.data(), 1, acc.size(), f);
    std::fclose(f);
    std::printf("refine_demo: %u x %u, %llu selected, %llu pixel-frames in %u passes\n", w, h,
                (unsigned long long)selected, (unsigned long long)res.pixel_frames, res.passes);
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "refine_demo: %s\n", e.what());
    rc = 10 + (int)e.status;
  }
  (void)hipFree(hits);
  return rc;
}
