// hrt_variance.hip -- gfx950 kernels of the variance-guided denoise (hrt_variance.h):
// variance_prep and the a-trous pass in its two kernels, atrous_variance_direct (every tap a global load) and
// atrous_variance_tiled (taps from a dense tile staged in LDS).
//
// S16 is pinned operation by operation and the unit is built with -ffp-contract=off: every statement of
// variance_estimate / var_prefilter_tap / var_centre / var_tap / var_store below is one rounded float operation
// of the spec, in its order.  Both pass kernels call the same functions and differ only in the loads that feed them.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hip_raytrace.h"
#include "hrt_math.h"
#include "hrt_variance.h"

namespace hrt {

constexpr uint32_t kTileW = 32, kTileH = 8;  // one pixel per thread of a 256-thread workgroup, a wave = 2 rows

// S14's surface key of a hit record's first 16 bytes {t, kind, index, mesh}.
__device__ __forceinline__ uint32_t var_key(float4 a) {
  const uint32_t kind = __float_as_uint(a.y), index = __float_as_uint(a.z), mesh = __float_as_uint(a.w);
  if (kind == 1u) return 0x80000000u | (index & 0x7FFFFFFFu);
  if (kind == 2u) return (mesh + 1u) & 0x7FFFFFFFu;
  return 0u;
}
// S14's C0 of a texel and S16's luminance of it.
__device__ __forceinline__ f3 var_c0(uint32_t v) {
  return {unorm8_to_float(v & 255u), unorm8_to_float((v >> 8) & 255u), unorm8_to_float((v >> 16) & 255u)};
}
__device__ __forceinline__ f3 var_c0(float4 v) { return {v.x, v.y, v.z}; }
__device__ __forceinline__ float var_lum(f3 c) { return variance_lum(c.x, c.y, c.z); }

// denoise_prep's job with V0 in the .w of C0.  One kernel, not a second one over the pixels without history: the
// temporal estimate is three operations on values the kernel holds anyway, and the pixels that take the 7 x 7
// spatial estimate (n < min_history) are the disocclusions of a move, contiguous regions, so whole waves take
// or skip the window; a second kernel would need a list of those pixels, built by a pass of its own over N.
template <typename T>
__global__ __launch_bounds__(256) void variance_prep(const T* __restrict__ src, const float4* __restrict__ hits,
                                                     const uint32_t* __restrict__ cnt, const float2* __restrict__ mom,
                                                     float4* __restrict__ c0, float4* __restrict__ guide,
                                                     uint32_t* __restrict__ keys, uint32_t w, uint32_t h,
                                                     uint32_t min_history) {
  const uint32_t x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1u));
  const uint32_t y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  if (x >= w || y >= h) return;
  const size_t i = (size_t)y * w + x;
  const f3 c = var_c0(src[i]);
  uint32_t key = 0u;
  if (hits) {
    const float4 a = hits[2 * i], b = hits[2 * i + 1];  // {t, kind, index, mesh}, {n.x, n.y, n.z, reserved}
    guide[i] = make_float4(b.x, b.y, b.z, a.x);
    key = var_key(a);
    keys[i] = key;
  }
  const uint32_t n = cnt[i];
  float v0;
  if (n >= min_history) {
    const float2 m = mom[i];
    const float d = m.y - m.x * m.x;
    const float tv = d > 0.0f ? d : 0.0f;
    v0 = tv / (float)n;
  } else {
    float s1 = 0.0f, s2 = 0.0f, k = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
      const int64_t qy = (int64_t)y + dy;
      if (qy < 0 || qy >= (int64_t)h) continue;
      for (int dx = -3; dx <= 3; ++dx) {
        const int64_t qx = (int64_t)x + dx;
        if (qx < 0 || qx >= (int64_t)w) continue;
        const size_t q = (size_t)qy * w + (size_t)qx;
        if (hits && var_key(hits[2 * q]) != key) continue;
        const float lq = var_lum(var_c0(src[q]));
        s1 = s1 + lq;
        s2 = s2 + lq * lq;
        k = k + 1.0f;
      }
    }
    const float mean = s1 / k;
    const float e = s2 / k - mean * mean;
    v0 = e > 0.0f ? e : 0.0f;
  }
  c0[i] = make_float4(c.x, c.y, c.z, v0);
}

// The centre pixel of a pass: its colour and variance, guide and the constants of S16 that depend on it.
struct VarCentre {
  float4 c, g;  // c.w = V_i(p)
  float kv, kn, kd;
  bool weigh;  // guided and key(p) != 0: wn and wd are computed
  float ar, ag, ab, vacc, wsum;
};

// G = {0.5, 0.25}: the 3 x 3 Gaussian's row.
__device__ __forceinline__ constexpr float var_g(int d) { return d == 0 ? 0.5f : 0.25f; }
// One tap of the prefilter that lies inside the image.
__device__ __forceinline__ void var_prefilter_tap(float& va, float& gs, float g, float vq) {
  va = va + g * vq;
  gs = gs + g;
}

__device__ __forceinline__ VarCentre var_centre(float4 c, float4 g, uint32_t key, bool guided, float va, float gs,
                                                float sv2, float variance_floor, float kn, float sigma_depth, float fs) {
  VarCentre p;
  p.c = c;
  p.g = g;
  const float vg = va / gs;
  p.kv = 1.0f / ((sv2 * vg) + variance_floor);
  p.kn = kn;
  p.weigh = guided && key != 0u;
  p.kd = p.weigh ? 1.0f / ((sigma_depth * g.w) * fs) : 0.0f;
  p.ar = p.ag = p.ab = p.vacc = p.wsum = 0.0f;
  return p;
}

// One tap that passed the skips (inside the image, same key).
__device__ __forceinline__ void var_tap(VarCentre& p, float h, float4 cq, float4 gq) {
  const float er = p.c.x - cq.x, eg = p.c.y - cq.y, eb = p.c.z - cq.z;
  const float dc = (er * er + eg * eg) + eb * eb;
  const float wc = 1.0f / (1.0f + dc * p.kv);
  float wn = 1.0f, wd = 1.0f;
  if (p.weigh) {
    const float dot = (p.g.x * gq.x + p.g.y * gq.y) + p.g.z * gq.z;
    const float a = 1.0f - (1.0f - dot) * p.kn;
    wn = a > 0.0f ? a : 0.0f;
    const float b = 1.0f - fabsf(p.g.w - gq.w) * p.kd;
    wd = b > 0.0f ? b : 0.0f;
  }
  const float w = ((h * wc) * wn) * wd;
  p.ar = p.ar + w * cq.x;
  p.ag = p.ag + w * cq.y;
  p.ab = p.ab + w * cq.z;
  p.vacc = p.vacc + (w * w) * cq.w;
  p.wsum = p.wsum + w;
}

// K = {0.375, 0.25, 0.0625}: the B3 spline row; every product of two entries is exact in binary32.
__device__ __forceinline__ constexpr float var_k(int d) {
  const int a = d < 0 ? -d : d;
  return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

// The store of a texel {r, g, b} with variance v in one of the three output forms (hrt_variance.h VarianceOut).
template <int OutKind>
__device__ __forceinline__ void var_write(void* out, float* vout, size_t i, float r, float g, float b, float v) {
  if constexpr (OutKind == kVarianceOutPass) {
    static_cast<float4*>(out)[i] = make_float4(r, g, b, v);
  } else {
    if constexpr (OutKind == kVarianceOutRgba8)
      static_cast<uint32_t*>(out)[i] = unorm8(r) | (unorm8(g) << 8) | (unorm8(b) << 16) | (255u << 24);
    else
      static_cast<float4*>(out)[i] = make_float4(r, g, b, 1.0f);
    if (vout) vout[i] = v;
  }
}
// The result of the pass.
template <int OutKind>
__device__ __forceinline__ void var_store(void* out, float* vout, size_t i, const VarCentre& p) {
  const float r = p.ar / p.wsum, g = p.ag / p.wsum, b = p.ab / p.wsum;
  const float v = p.vacc / (p.wsum * p.wsum);
  var_write<OutKind>(out, vout, i, r, g, b, v);
}

// The literal form: one thread per pixel; the nine prefilter taps and every tap's colour, guide and key are
// global loads.
template <bool Guided, int OutKind>
__global__ __launch_bounds__(256) void atrous_variance_direct(const float4* __restrict__ cin, const float4* __restrict__ guide,
                                                              const uint32_t* __restrict__ keys, void* __restrict__ out,
                                                              float* __restrict__ vout, uint32_t w, uint32_t h, uint32_t s,
                                                              float sv2, float variance_floor, float kn, float sigma_depth) {
  const uint32_t x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1u));
  const uint32_t y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  if (x >= w || y >= h) return;
  const size_t i = (size_t)y * w + x;
  float va = 0.0f, gs = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    const int64_t qy = (int64_t)y + dy;
    if (qy < 0 || qy >= (int64_t)h) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int64_t qx = (int64_t)x + dx;
      if (qx < 0 || qx >= (int64_t)w) continue;
      var_prefilter_tap(va, gs, var_g(dx) * var_g(dy), cin[(size_t)qy * w + (size_t)qx].w);
    }
  }
  const uint32_t key = Guided ? keys[i] : 0u;
  VarCentre p = var_centre(cin[i], Guided ? guide[i] : float4{}, key, Guided, va, gs, sv2, variance_floor, kn, sigma_depth,
                           (float)s);
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int64_t qy = (int64_t)y + (int64_t)s * dy;
    if (qy < 0 || qy >= (int64_t)h) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int64_t qx = (int64_t)x + (int64_t)s * dx;
      if (qx < 0 || qx >= (int64_t)w) continue;
      const size_t q = (size_t)qy * w + (size_t)qx;
      if (Guided && keys[q] != key) continue;
      var_tap(p, var_k(dx) * var_k(dy), cin[q], Guided ? guide[q] : float4{});
    }
  }
  var_store<OutKind>(out, vout, i, p);
}

// The tiled form.  A workgroup takes a kTileW x kTileH tile of the image; the tile and its halo of 2 s pixels --
// {r, g, b, V}, guide and key of every pixel inside the image -- are staged in dynamic LDS with one 16-byte load
// per array and pixel, then every tap and the nine prefilter taps (one pixel apart: inside the halo at every
// step, 2 s >= 1) are LDS reads.  Pixels outside the image are never staged and never read (the bounds test is
// on the coordinates, as in atrous_variance_direct).
template <bool Guided, int OutKind>
__global__ __launch_bounds__(256) void atrous_variance_tiled(const float4* __restrict__ cin, const float4* __restrict__ guide,
                                                             const uint32_t* __restrict__ keys, void* __restrict__ out,
                                                             float* __restrict__ vout, uint32_t w, uint32_t h, uint32_t s,
                                                             float sv2, float variance_floor, float kn, float sigma_depth) {
  extern __shared__ float4 lds[];
  const uint32_t r = 2u * s;
  const uint32_t lw = kTileW + 2u * r, lh = kTileH + 2u * r, n = lw * lh;
  float4* sc = lds;
  float4* sg = lds + n;                                                // (guided only)
  uint32_t* sk = reinterpret_cast<uint32_t*>(lds + 2u * (size_t)n);  // (guided only)
  // the tile's first pixel less the halo (may be negative)
  const int64_t ox = (int64_t)blockIdx.x * kTileW - (int64_t)r;
  const int64_t oy = (int64_t)blockIdx.y * kTileH - (int64_t)r;
  for (uint32_t e = threadIdx.x; e < n; e += 256u) {
    const uint32_t j = e / lw, i = e - j * lw;
    const int64_t px = ox + i, py = oy + j;
    if (px < 0 || px >= (int64_t)w || py < 0 || py >= (int64_t)h) continue;
    const size_t q = (size_t)py * w + (size_t)px;
    sc[e] = cin[q];
    if (Guided) {
      sg[e] = guide[q];
      sk[e] = keys[q];
    }
  }
  __syncthreads();
  const uint32_t li = r + (threadIdx.x & (kTileW - 1u)), lj = r + threadIdx.x / kTileW;
  const int64_t x = ox + li, y = oy + lj;  // >= 0
  if (x >= (int64_t)w || y >= (int64_t)h) return;
  const uint32_t ce = lj * lw + li;
  float va = 0.0f, gs = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    const int64_t qy = y + dy;
    if (qy < 0 || qy >= (int64_t)h) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int64_t qx = x + dx;
      if (qx < 0 || qx >= (int64_t)w) continue;
      var_prefilter_tap(va, gs, var_g(dx) * var_g(dy), sc[(uint32_t)((int)lj + dy) * lw + (uint32_t)((int)li + dx)].w);
    }
  }
  const uint32_t key = Guided ? sk[ce] : 0u;
  VarCentre p = var_centre(sc[ce], Guided ? sg[ce] : float4{}, key, Guided, va, gs, sv2, variance_floor, kn, sigma_depth,
                           (float)s);
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int64_t qy = y + (int64_t)s * dy;
    if (qy < 0 || qy >= (int64_t)h) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int64_t qx = x + (int64_t)s * dx;
      if (qx < 0 || qx >= (int64_t)w) continue;
      const uint32_t e = (uint32_t)((int)lj + (int)s * dy) * lw + (uint32_t)((int)li + (int)s * dx);
      if (Guided && sk[e] != key) continue;
      var_tap(p, var_k(dx) * var_k(dy), sc[e], Guided ? sg[e] : float4{});
    }
  }
  var_store<OutKind>(out, vout, (size_t)y * w + (size_t)x, p);
}

// iterations == 0: C0 and V0 in the output form.
template <int OutKind>
__global__ __launch_bounds__(256) void variance_store(const float4* __restrict__ in, void* __restrict__ out,
                                                      float* __restrict__ vout, size_t npix) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= npix) return;
  const float4 c = in[i];
  var_write<OutKind>(out, vout, i, c.x, c.y, c.z, c.w);
}

constexpr size_t kTiledMaxLds = 64u << 10;  // the dynamic LDS a launch may ask for without an attribute

hipError_t launch_variance_prep(const VariancePrep& p, hipStream_t stream) {
  if (p.w == 0 || p.h == 0) return hipSuccess;
  if (!p.src || !p.cnt || !p.mom || !p.c0 || (p.hits && (!p.guide || !p.keys)) || p.min_history == 0)
    return hipErrorInvalidValue;
  if ((((uintptr_t)p.c0 | (uintptr_t)p.hits | (uintptr_t)p.guide) & 15u) != 0 || ((uintptr_t)p.mom & 7u) != 0)
    return hipErrorInvalidValue;
  const dim3 grid((p.w + kTileW - 1) / kTileW, (p.h + kTileH - 1) / kTileH, 1);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  const float4* hp = reinterpret_cast<const float4*>(p.hits);
  const float2* mp = reinterpret_cast<const float2*>(p.mom);
  if (p.f32)
    variance_prep<float4><<<grid, 256, 0, stream>>>(static_cast<const float4*>(p.src), hp, p.cnt, mp, static_cast<float4*>(p.c0),
                                                    static_cast<float4*>(p.guide), static_cast<uint32_t*>(p.keys), p.w, p.h,
                                                    p.min_history);
  else
    variance_prep<uint32_t><<<grid, 256, 0, stream>>>(static_cast<const uint32_t*>(p.src), hp, p.cnt, mp,
                                                      static_cast<float4*>(p.c0), static_cast<float4*>(p.guide),
                                                      static_cast<uint32_t*>(p.keys), p.w, p.h, p.min_history);
  return hipGetLastError();
}

template <bool Guided, int OutKind>
static hipError_t variance_atrous_launch(const VariancePass& p, int form, hipStream_t stream) {
  const float4* cin = static_cast<const float4*>(p.in);
  const float4* gd = static_cast<const float4*>(p.guide);
  const uint32_t* keys = static_cast<const uint32_t*>(p.keys);
  const dim3 grid((p.w + kTileW - 1) / kTileW, (p.h + kTileH - 1) / kTileH, 1);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  if (form == kVarianceDirect) {
    atrous_variance_direct<Guided, OutKind><<<grid, 256, 0, stream>>>(cin, gd, keys, p.out, p.vout, p.w, p.h, p.step, p.sv2,
                                                                      p.variance_floor, p.kn, p.sigma_depth);
    return hipGetLastError();
  }
  const uint32_t r = 2u * p.step;
  const size_t n = (size_t)(kTileW + 2u * r) * (kTileH + 2u * r);
  const size_t bytes = n * (Guided ? 36u : 16u);
  if (bytes > kTiledMaxLds) return hipErrorInvalidValue;
  atrous_variance_tiled<Guided, OutKind><<<grid, 256, bytes, stream>>>(cin, gd, keys, p.out, p.vout, p.w, p.h, p.step, p.sv2,
                                                                       p.variance_floor, p.kn, p.sigma_depth);
  return hipGetLastError();
}

template <bool Guided>
static hipError_t variance_atrous_kind(const VariancePass& p, int form, hipStream_t stream) {
  if (p.out_kind == kVarianceOutPass) return variance_atrous_launch<Guided, kVarianceOutPass>(p, form, stream);
  if (p.out_kind == kVarianceOutFloat) return variance_atrous_launch<Guided, kVarianceOutFloat>(p, form, stream);
  return variance_atrous_launch<Guided, kVarianceOutRgba8>(p, form, stream);
}

hipError_t launch_variance_atrous(const VariancePass& p, int form, hipStream_t stream) {
  if (p.w == 0 || p.h == 0) return hipSuccess;
  if (!p.in || !p.out || p.in == p.out || (p.guide == nullptr) != (p.keys == nullptr)) return hipErrorInvalidValue;
  if (p.step == 0 || p.step > (1u << (kVarianceMaxIterations - 1)) || (p.step & (p.step - 1u)) != 0) return hipErrorInvalidValue;
  if (form != kVarianceDirect && form != kVarianceTiled) return hipErrorInvalidValue;
  if (p.out_kind != kVarianceOutPass && p.out_kind != kVarianceOutFloat && p.out_kind != kVarianceOutRgba8)
    return hipErrorInvalidValue;
  if (p.out_kind == kVarianceOutPass && p.vout) return hipErrorInvalidValue;
  return p.guide ? variance_atrous_kind<true>(p, form, stream) : variance_atrous_kind<false>(p, form, stream);
}

hipError_t launch_variance_store(const void* in, void* out, float* vout, int out_kind, size_t npix, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  if (!in || !out || in == out) return hipErrorInvalidValue;
  const unsigned int grid = (unsigned int)((npix + 255) / 256);
  const float4* cin = static_cast<const float4*>(in);
  if (out_kind == kVarianceOutFloat)
    variance_store<kVarianceOutFloat><<<grid, 256, 0, stream>>>(cin, out, vout, npix);
  else if (out_kind == kVarianceOutRgba8)
    variance_store<kVarianceOutRgba8><<<grid, 256, 0, stream>>>(cin, out, vout, npix);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hrt
