// oracle/glsl_ref/selfcheck_main.cpp -- run by oracle/Makefile right after the translated shaders are built: the build
// fails unless the compiler evaluated the two RNG draws of raytracing.glsl:164 left to right (rt_harness.inc,
// glr_selfcheck).  clang++ does; g++ evaluates the operands of an overloaded `+` right to left and fails here.
#include <cstdio>

extern "C" int glr_selfcheck(void);

int main() {
  int r = glr_selfcheck();
  if (r == 0) return 0;
  if (r < 0)
    std::fprintf(stderr, "glsl_ref selfcheck: the probe cannot tell the two evaluation orders apart\n");
  else
    std::fprintf(stderr, "glsl_ref selfcheck: get_ray_dir's draws are not evaluated left to right on %d of 4096 states "
                         "(build the translated shaders with clang++)\n", r);
  return 1;
}
