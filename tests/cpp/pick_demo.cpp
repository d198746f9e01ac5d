// Ray queries through include/hrt_app.hpp, the C++ mirror of the host surface: RayTracePipeline::first_hits of
// a whole view, then RayTracePipeline::pick of its centre pixel and of pixel (0, 0).
// tests/test_gpu_intersect.py asks the Python mirror the same and compares the records.
//
//   pick_demo <out.bin> <width> <height>
//
// Scene and camera: app_demo.cpp's (mirrored in tests/test_cpp_app.py::demo_settings, no OBJ file).  Output:
// u32 width, u32 height, width x height hrt_hit records (row-major, trace-image rows), the two picks.  A library
// error prints its message and exits with 10 + the hrt_status.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hrt_app.hpp"

static epq::RayTracerSettings demo_settings() {
  epq::RayTracerSettings s;
  s.num_samples = 1;
  s.max_bounces = 1;
  s.use_environment_lighting = true;
  s.sphere_data = {
      epq::Sphere{{0.0f, -100.5f, -1.0f}, 100.0f, epq::LambertianMaterial{{0.8f, 0.8f, 0.0f}}},
      epq::Sphere{{0.0f, 0.0f, -1.2f}, 0.5f, epq::MetalMaterial{{0.8f, 0.6f, 0.2f}, 0.9f, 0.05f}},
      epq::Sphere{{-1.0f, 0.3f, -1.0f}, 0.3f, epq::LightMaterial{{1.0f, 0.9f, 0.7f, 4.0f}}},
      epq::Sphere{{1.2f, 1.5f, -0.5f}, 0.4f, epq::InvisLightMaterial{{0.9f, 0.9f, 1.0f, 6.0f}}},
  };
  epq::CustomMaterial quad_mat;
  quad_mat.colour = {0.2f, 0.5f, 0.8f};
  quad_mat.smoothness = 0.3f;
  quad_mat.specular_probability = 0.25f;
  s.mesh_data.push_back(epq::RayTracingMesh{
      epq::Mesh{{0.5f, -0.5f, -2.0f, 1.5f, -0.5f, -2.0f, 1.5f, 0.8f, -2.0f, 0.5f, 0.8f, -2.0f}, {0, 1, 2, 0, 2, 3}, "quad"},
      quad_mat});
  return s;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s out.bin width height\n", argv[0]);
    return 2;
  }
  const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
  try {
    epq::Camera cam;
    cam.position = {0.0f, 0.3f, 1.5f};
    cam.direction = {0.0f, -0.1f, -1.0f};
    epq::Context ctx(w, h, -1, HRT_MODE_RGBA8);
    epq::RayTracePipeline pipe(ctx, {w, h}, demo_settings());
    const std::vector<hrt_hit> first = pipe.first_hits(cam);
    const hrt_hit picks[2] = {pipe.pick(cam, w / 2, h / 2), pipe.pick(cam, 0, 0)};
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    std::fwrite(&w, 4, 1, f);
    std::fwrite(&h, 4, 1, f);
    std::fwrite(first.data(), sizeof(hrt_hit), first.size(), f);
    std::fwrite(picks, sizeof(hrt_hit), 2, f);
    std::fclose(f);
    std::printf("pick_demo: %ux%u first hits; the centre pixel sees kind %u, index %u at t = %g\n", w, h, picks[0].kind,
                picks[0].index, (double)picks[0].t);
    return 0;
  } catch (const epq::HrtError& e) {
    std::fprintf(stderr, "pick_demo: %s\n", e.what());
    return 10 + (int)e.status;
  }
}
