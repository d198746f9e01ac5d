// The first-hit pass through include/hrt_app.hpp, the C++ mirror of the host surface: the first hits of a 48 x 32
// view from two cameras enqueued into two device buffers (RayTracePipeline::first_hits_enqueue, TILES with
// counting, then QUERY), one Context::synchronize, and the buffers copied back.
// tests/test_gpu_first_hits.py compares the bytes with the Python mirror's on the same scene.
//
//   first_hits_demo <in.bin> <out.bin>
//
// Input: history_demo's format (u32 spheres, per sphere centre and radius; u32 meshes, per mesh u32 vertices,
// u32 indices, the positions, the indices); every primitive Lambertian grey.
// Output: u32 width, u32 height, the hrt_first_hits_stats of the counted TILES call, then the two hit images.
// A library error prints its message and exits with 10 + the hrt_status.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hrt_app.hpp"

// the HIP runtime calls the demo needs for its device buffers (hrt_app.hpp itself is HIP-free)
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
  int rc = 0;
  try {
    const uint32_t w = 48, h = 32, npix = w * h;
    epq::Context ctx(w, h, -1, HRT_MODE_RGBA32F);
    epq::RayTracePipeline pipe(ctx, {w, h}, s);
    const epq::Camera before{};
    epq::Camera after{};
    after.position = {0.05f, 0.02f, -0.03f};
    after.direction = {1.0f, 0.03f, 0.08f};
    for (void*& p : hits)
      if (hipMalloc(&p, (size_t)npix * sizeof(hrt_hit)) != 0) return 5;
    pipe.first_hits_enqueue(before, static_cast<hrt_hit*>(hits[0]), HRT_FIRST_HITS_TILES, true);
    pipe.first_hits_enqueue(after, static_cast<hrt_hit*>(hits[1]), HRT_FIRST_HITS_QUERY);
    ctx.synchronize();
    const hrt_first_hits_stats st = ctx.first_hits_stats();
    std::vector<hrt_hit> host((size_t)2 * npix);
    for (int i = 0; i < 2; ++i)
      if (hipMemcpy(host.data() + (size_t)i * npix, hits[i], (size_t)npix * sizeof(hrt_hit), 2) != 0) return 5;
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(&w, 4, 1, f);
    std::fwrite(&h, 4, 1, f);
    std::fwrite(&st, sizeof st, 1, f);
    std::fwrite(host.data(), sizeof(hrt_hit), host.size(), f);
    std::fclose(f);
    std::printf("first_hits_demo: %u x %u, %u tiles (%u listed)\n", w, h, st.tiles, st.tiles_listed);
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "first_hits_demo: %s\n", e.what());
    rc = 10 + (int)e.status;
  }
  (void)hipFree(hits[0]);
  (void)hipFree(hits[1]);
  return rc;
}
