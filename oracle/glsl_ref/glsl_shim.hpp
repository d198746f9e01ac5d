// oracle/glsl_ref/glsl_shim.hpp -- the slice of GLSL 4.60 that the reference's two compute shaders use, as C++20.
//
// TEST INFRASTRUCTURE ONLY.  translate.py rewrites assets/raytracing.glsl and assets/image_combiner.glsl of the
// reference checkout mechanically into oracle/_ref/ (never committed) and compiles them against this header, so that
// the oracle and the HIP kernels can be compared with the shader's own statements.  This header holds none of the
// shader's text and none of rt_oracle.c's: every builtin below is written from the rule in DESIGN.md 2 --
//   S1  IEEE binary32, round to nearest even, denormals kept (build: -ffp-contract=off -fno-fast-math);
//   S2  dot, cross, mat3 * vec3 are the FMA chains spelled out below;
//   S4  '/' and sqrt are the correctly rounded ones; normalize(v) = v / sqrt(dot(v, v)), three divisions;
//   S5  log / sin / cos are the oracle library's exported spec_logf / spec_sinf / spec_cosf (tests/test_oracle.py
//       pins those to libm);
//   S6  min(x, y) = y < x ? y : x, max(x, y) = x < y ? y : x, mix(x, y, a) = x * (1 - a) + y * a,
//       reflect(I, N) = I - (2 * dot(N, I)) * N;
//   S7  an rgba8 image stores NaN and x <= 0 as 0, x >= 1 as 255, else rint(x * 255); it loads k / 255.
// Everything else (vector + - * /, scalar broadcasts) is one IEEE operation per component, in the written order.
//
// Evaluation order: GLSL evaluates operands left to right; C++ leaves the order of an overloaded
// operator's operands to the compiler.  The recipe therefore builds with clang++ and then RUNS a check of the one
// expression with two RNG draws in it (selfcheck in rt_harness.inc); a compiler that orders them otherwise fails
// the build.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

extern "C" {
float spec_logf(float);
float spec_sinf(float);
float spec_cosf(float);
}

namespace glsl {

using uint = std::uint32_t;

struct vec4;

struct vec3 {
  float x, y, z;
  vec3() = default;
  explicit vec3(float s) : x(s), y(s), z(s) {}
  vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
  explicit vec3(const vec4& v);
  vec3& operator+=(vec3 b) { x = x + b.x; y = y + b.y; z = z + b.z; return *this; }
  vec3& operator*=(vec3 b) { x = x * b.x; y = y * b.y; z = z * b.z; return *this; }
  vec3& operator/=(float s) { x = x / s; y = y / s; z = z / s; return *this; }
};

struct vec4 {
  float x, y, z, w;
  vec4() = default;
  explicit vec4(float s) : x(s), y(s), z(s), w(s) {}
  vec4(float x_, float y_, float z_, float w_) : x(x_), y(y_), z(z_), w(w_) {}
  vec4(vec3 v, float w_) : x(v.x), y(v.y), z(v.z), w(w_) {}
  vec3 xyz() const { return vec3(x, y, z); }
};

inline vec3::vec3(const vec4& v) : x(v.x), y(v.y), z(v.z) {}

struct ivec2 {
  int x, y;
  ivec2() = default;
  ivec2(int x_, int y_) : x(x_), y(y_) {}
  ivec2(uint x_, uint y_) : x(int(x_)), y(int(y_)) {}
};

struct uvec3 { uint x, y, z; };

// column-major, as std430 lays a matrix out: c[k] is column k
struct mat4 { float c[4][4]; };
struct mat3 {
  float c[3][3];
  explicit mat3(const mat4& m) {
    for (int k = 0; k < 3; k++)
      for (int r = 0; r < 3; r++) c[k][r] = m.c[k][r];
  }
};

// a std430 / push-constant bool: one 32-bit word, true when nonzero
struct bool32 {
  uint v;
  operator bool() const { return v != 0u; }
};

// ---- componentwise arithmetic: one IEEE operation per component ---------------------------------------------------
inline vec3 operator-(vec3 a) { return vec3(-a.x, -a.y, -a.z); }
inline vec3 operator+(vec3 a, vec3 b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(vec3 a, vec3 b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(vec3 a, vec3 b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator/(vec3 a, vec3 b) { return vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline vec3 operator+(vec3 a, float s) { return vec3(a.x + s, a.y + s, a.z + s); }
inline vec3 operator*(vec3 a, float s) { return vec3(a.x * s, a.y * s, a.z * s); }
inline vec3 operator*(float s, vec3 a) { return vec3(s * a.x, s * a.y, s * a.z); }
inline vec3 operator/(vec3 a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }

// ---- S2 ----------------------------------------------------------------------------------------------------------
inline float dot(vec3 a, vec3 b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }
inline vec3 cross(vec3 a, vec3 b) {
  return vec3(std::fmaf(a.y, b.z, -(a.z * b.y)), std::fmaf(a.z, b.x, -(a.x * b.z)), std::fmaf(a.x, b.y, -(a.y * b.x)));
}
inline vec3 operator*(const mat3& m, vec3 v) {
  float r[3];
  for (int i = 0; i < 3; i++) r[i] = std::fmaf(m.c[2][i], v.z, std::fmaf(m.c[1][i], v.y, m.c[0][i] * v.x));
  return vec3(r[0], r[1], r[2]);
}

// ---- S4 ----------------------------------------------------------------------------------------------------------
inline float sqrt(float x) { return std::sqrt(x); }
inline vec3 normalize(vec3 v) { return v / glsl::sqrt(dot(v, v)); }

// ---- S5 ----------------------------------------------------------------------------------------------------------
inline float log(float x) { return spec_logf(x); }
inline float sin(float x) { return spec_sinf(x); }
inline float cos(float x) { return spec_cosf(x); }

// ---- S6 ----------------------------------------------------------------------------------------------------------
inline float min(float x, float y) { return (y < x) ? y : x; }
inline float max(float x, float y) { return (x < y) ? y : x; }
inline vec3 mix(vec3 x, vec3 y, float a) { return x * (1.0f - a) + y * a; }
inline vec3 reflect(vec3 I, vec3 N) { return I - (2.0f * dot(N, I)) * N; }

// ---- S7: an rgba8 storage image, with a float side channel holding what was stored before quantisation ------------
inline std::uint8_t unorm8_store(float x) {
  if (!(x > 0.0f)) return 0;  // NaN, zeros, negatives
  if (x >= 1.0f) return 255;
  return std::uint8_t(int(std::rint(x * 255.0f)));
}
inline float unorm8_load(std::uint8_t k) { return float(k) / 255.0f; }

struct image2D {
  std::uint8_t* texels = nullptr;  // width * height * 4
  float* stored = nullptr;         // optional: the vec4 of the last imageStore per texel
  uint width = 0, height = 0;
};
inline void imageStore(image2D& im, ivec2 p, vec4 v) {
  if (p.x < 0 || p.y < 0 || uint(p.x) >= im.width || uint(p.y) >= im.height) return;  // out-of-image stores are dropped
  std::size_t k = (std::size_t(p.y) * im.width + std::size_t(p.x)) * 4;
  const float f[4] = {v.x, v.y, v.z, v.w};
  for (int c = 0; c < 4; c++) {
    if (im.texels) im.texels[k + c] = unorm8_store(f[c]);
    if (im.stored) im.stored[k + c] = f[c];
  }
}
inline vec4 imageLoad(const image2D& im, ivec2 p) {
  if (p.x < 0 || p.y < 0 || uint(p.x) >= im.width || uint(p.y) >= im.height) return vec4(0.0f);
  const std::uint8_t* t = im.texels + (std::size_t(p.y) * im.width + std::size_t(p.x)) * 4;
  return vec4(unorm8_load(t[0]), unorm8_load(t[1]), unorm8_load(t[2]), unorm8_load(t[3]));
}

// ---- a storage buffer whose reads are counted (the shader's own triangle-test count) ------------------------------
template <class T>
struct counted_buffer {
  const T* data = nullptr;
  std::uint64_t reads = 0;
  const T& operator[](uint i) { reads++; return data[i]; }
};

}  // namespace glsl
