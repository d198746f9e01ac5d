// oracle/glsl_ref/combiner_harness.inc -- C ABI around the translated image combiner (appended to the generated unit
// by translate.py; see glsl_shim.hpp).  This project's own code: it holds none of the shader's text.
namespace C = glsl::image_combiner;

static_assert(sizeof(C::PushConstants) == 12, "combiner push constants");

extern "C" {

// One fold (image_combiner.glsl:22-43) of `new_image` into `current`, both width * height rgba8 texels, as frame
// number `frame`.  main() runs for x < width and y < height only; the shader's `>` bound (:27) is the same harmless
// quirk as the path tracer's.
void glr_combine_rgba8(uint32_t frame, uint8_t* current, const uint8_t* new_image, uint32_t width, uint32_t height) {
  C::push_constants.frame = frame;
  C::push_constants.image_width = width;
  C::push_constants.image_height = height;
  C::current_image = glsl::image2D{current, nullptr, width, height};
  C::new_image = glsl::image2D{const_cast<uint8_t*>(new_image), nullptr, width, height};  // only loaded from
  for (uint32_t y = 0; y < height; y++)
    for (uint32_t x = 0; x < width; x++) {
      C::gl_GlobalInvocationID = glsl::uvec3{x, y, 0};
      C::shader_main();
    }
}

}  // extern "C"
