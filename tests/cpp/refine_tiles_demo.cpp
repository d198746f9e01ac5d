// Tile-masked refinement through include/hrt_app.hpp, the C++ mirror of the host surface: on a 48 x 32 view traced by
// BUNDLE_WQ, Context::refine_tiles gives the pixels of the image's left half the frames 0 and 1 in one pass, then
// Context::refine_tiles_until runs two passes of two frames each (the frames 2..5) under the default rule.
// tests/test_gpu_refine_tiles.py runs the Python mirror on the same scene and compares the bytes.
//
//   refine_tiles_demo <in.bin> <out.bin>
//
// Input (little-endian, written by the test from the Python scene): u32 spheres, per sphere 4 floats (centre,
// radius); u32 meshes, per mesh u32 vertices, u32 indices, the positions, the indices.  Every primitive is
// Lambertian grey; 1 sample, 4 bounces, environment light on, RGBA32F.
// Output: eight u64 -- width, height, the first pass's tiles, selected tiles, selected pixels and traced pixels, the
// loop's passes and pixel-frames -- then the count image and the accumulator (RGBA32F).  A library error prints its
// message and exits with 10 + the hrt_status.
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
    const uint32_t w = 48, h = 32;
    epq::Context ctx(w, h, -1, HRT_MODE_RGBA32F);
    ctx.set_option(HRT_OPT_KERNEL_VARIANT, HRT_KERNEL_BUNDLE_WQ);
    epq::RayTracePipeline pipe(ctx, {w, h}, s);
    epq::Camera cam{};
    cam.position = {3.0f, 1.5f, 2.0f};
    cam.direction = {-0.8f, -0.3f, -0.6f};
    std::vector<uint32_t> mask(ctx.mask_words(), 0u);
    for (uint32_t y = 0; y < h; ++y)
      for (uint32_t x = 0; x < w / 2; ++x) mask[(x + y * w) >> 5] |= 1u << ((x + y * w) & 31u);
    const hrt_refine_tiles_stats st = ctx.refine_tiles(pipe.push_constants(cam, 0, false), mask.data(), HRT_HISTORY_MAX, 2);
    const epq::Context::RefineResult res = ctx.refine_tiles_until(pipe.push_constants(cam, 2, false),
                                                                  epq::Context::refine_defaults(), nullptr, HRT_HISTORY_MAX, 2, 2);
    const std::vector<uint32_t> counts = ctx.read_history();
    const std::vector<uint8_t> acc = ctx.read(HRT_IMG_ACCUM, HRT_FMT_RGBA32F);
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    const uint64_t head[8] = {w, h, st.tiles, st.tiles_selected, st.selected, st.pixels_traced, res.passes, res.pixel_frames};
    std::fwrite(head, 8, 8, f);
    std::fwrite(counts.data(), 4, counts.size(), f);
    std::fwrite(acc.data(), 1, acc.size(), f);
    std::fclose(f);
    std::printf("refine_tiles_demo: %u x %u, %u of %u tiles in the first pass, %llu pixel-frames in %u passes\n", w, h,
                st.tiles_selected, st.tiles, (unsigned long long)res.pixel_frames, res.passes);
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "refine_tiles_demo: %s\n", e.what());
    rc = 10 + (int)e.status;
  }
  return rc;
}
