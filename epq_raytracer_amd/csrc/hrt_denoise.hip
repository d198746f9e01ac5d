// hrt_denoise.hip -- gfx950 kernels of the denoise pass (hrt_denoise.h): denoise_prep
// and the a-trous pass in its two kernels, atrous_direct (every tap a global load) and atrous_tiled (taps
// from a tile staged in LDS, dense or on the sub-lattice of the step).
//
// S14 is pinned operation by operation and the unit is built with -ffp-contract=off: every statement of
// atrous_centre / atrous_tap / atrous_store below is one rounded float operation of the spec, in its order.  Both kernels
// call the same three functions and differ only in the loads that feed them.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hip_raytrace.h"
#include "hrt_denoise.h"
#include "hrt_math.h"

namespace hrt {

constexpr uint32_t kTileW = 32, kTileH = 8;  // one pixel per thread of a 256-thread workgroup, a wave = 2 rows

// S14's surface key of a hit record's first 16 bytes {t, kind, index, mesh}.
__device__ __forceinline__ uint32_t surface_key(uint32_t kind, uint32_t index, uint32_t mesh) {
  if (kind == 1u) return 0x80000000u | (index & 0x7FFFFFFFu);
  if (kind == 2u) return (mesh + 1u) & 0x7FFFFFFFu;
  return 0u;
}

template <typename T>
__global__ __launch_bounds__(256) void denoise_prep(const T* __restrict__ src, const float4* __restrict__ hits,
                                                    float4* __restrict__ c0, float4* __restrict__ guide,
                                                    uint32_t* __restrict__ keys, size_t npix) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= npix) return;
  if constexpr (std::is_same_v<T, uint32_t>) {
    const uint32_t v = src[i];
    c0[i] = make_float4(unorm8_to_float(v & 255u), unorm8_to_float((v >> 8) & 255u), unorm8_to_float((v >> 16) & 255u),
                        1.0f);
  } else {
    c0[i] = src[i];
  }
  if (hits) {
    const float4 a = hits[2 * i], b = hits[2 * i + 1];  // {t, kind, index, mesh}, {n.x, n.y, n.z, reserved}
    guide[i] = make_float4(b.x, b.y, b.z, a.x);
    keys[i] = surface_key(__float_as_uint(a.y), __float_as_uint(a.z), __float_as_uint(a.w));
  }
}

// The centre pixel of a pass: its colour, guide and the constants of S14 that depend on it.
struct AtrousCentre {
  float4 c, g;
  float kc, kn, kd;
  bool weigh;  // guided and key(p) != 0: wn and wd are computed
  float ar, ag, ab, wsum;
};

// One tap that passed the skips (inside the image, same key): S14 step 5.
__device__ __forceinline__ void atrous_tap(AtrousCentre& p, float h, float4 cq, float4 gq) {
  const float er = p.c.x - cq.x, eg = p.c.y - cq.y, eb = p.c.z - cq.z;
  const float dc = (er * er + eg * eg) + eb * eb;
  const float wc = 1.0f / (1.0f + dc * p.kc);
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
  p.wsum = p.wsum + w;
}

__device__ __forceinline__ AtrousCentre atrous_centre(float4 c, float4 g, uint32_t key, bool guided, float kc, float kn,
                                                      float sigma_depth, float fs) {
  AtrousCentre p;
  p.c = c;
  p.g = g;
  p.kc = kc;
  p.kn = kn;
  p.weigh = guided && key != 0u;
  p.kd = p.weigh ? 1.0f / ((sigma_depth * g.w) * fs) : 0.0f;
  p.ar = p.ag = p.ab = p.wsum = 0.0f;
  return p;
}

// K = {0.375, 0.25, 0.0625}: the B3 spline row; every product of two entries is exact in binary32.
__device__ __forceinline__ constexpr float atrous_k(int d) {
  const int a = d < 0 ? -d : d;
  return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

// S14 step 6 and the store: a float4 texel with alpha 1.0f, or S7's RGBA8 word with alpha 255.
template <typename Out>
__device__ __forceinline__ void atrous_store(Out* out, size_t i, const AtrousCentre& p) {
  const float r = p.ar / p.wsum, g = p.ag / p.wsum, b = p.ab / p.wsum;
  if constexpr (std::is_same_v<Out, uint32_t>)
    out[i] = unorm8(r) | (unorm8(g) << 8) | (unorm8(b) << 16) | (255u << 24);
  else
    out[i] = make_float4(r, g, b, 1.0f);
}

// The literal form: one thread per pixel, every tap's colour, guide and key a global load.
template <bool Guided, typename Out>
__global__ __launch_bounds__(256) void atrous_direct(const float4* __restrict__ cin, const float4* __restrict__ guide,
                                                     const uint32_t* __restrict__ keys, Out* __restrict__ out,
                                                     uint32_t w, uint32_t h, uint32_t s, float kc, float kn,
                                                     float sigma_depth) {
  const uint32_t x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1u));
  const uint32_t y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  if (x >= w || y >= h) return;
  const size_t i = (size_t)y * w + x;
  const uint32_t key = Guided ? keys[i] : 0u;
  AtrousCentre p = atrous_centre(cin[i], Guided ? guide[i] : float4{}, key, Guided, kc, kn, sigma_depth, (float)s);
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
      atrous_tap(p, atrous_k(dx) * atrous_k(dy), cin[q], Guided ? guide[q] : float4{});
    }
  }
  atrous_store(out, i, p);
}

// The tiled form.  A workgroup takes a kTileW x kTileH tile of the lattice {(rx + lat i, ry + lat j)}: lat == 1
// is the image itself (the dense tile, halo 2s), lat == s the pixels congruent to (rx, ry) mod s, whose taps
// are their lattice neighbours (halo 2) at the price of global loads s pixels apart.  The tile and its halo of
// R = 2 s / lat lattice points -- colour, guide and key of every point inside the image -- are staged in
// dynamic LDS with one 16-byte load per array and point, then every tap is an LDS read: a lane reads the
// 16 bytes next to its neighbour's (ds_read_b128 over consecutive slots: no bank conflict), the same shift
// for every lane.  Points outside the image are never staged and never read (the bounds test is on the
// coordinates, as in atrous_direct).
template <bool Guided, typename Out>
__global__ __launch_bounds__(256) void atrous_tiled(const float4* __restrict__ cin, const float4* __restrict__ guide,
                                                    const uint32_t* __restrict__ keys, Out* __restrict__ out,
                                                    uint32_t w, uint32_t h, uint32_t s, uint32_t lat, float kc,
                                                    float kn, float sigma_depth) {
  extern __shared__ float4 lds[];
  const uint32_t m = s / lat, r = 2u * m;  // tap stride and halo, in lattice points
  const uint32_t lw = kTileW + 2u * r, lh = kTileH + 2u * r, n = lw * lh;
  float4* sc = lds;
  float4* sg = lds + n;                                                // (guided only)
  uint32_t* sk = reinterpret_cast<uint32_t*>(lds + 2u * (size_t)n);  // (guided only)
  const uint32_t rx = blockIdx.x % lat, ry = blockIdx.y % lat;
  // the tile's first lattice point, in pixels, less the halo (may be negative)
  const int64_t ox = (int64_t)rx + (int64_t)lat * ((int64_t)(blockIdx.x / lat) * kTileW - (int64_t)r);
  const int64_t oy = (int64_t)ry + (int64_t)lat * ((int64_t)(blockIdx.y / lat) * kTileH - (int64_t)r);
  for (uint32_t e = threadIdx.x; e < n; e += 256u) {
    const uint32_t j = e / lw, i = e - j * lw;
    const int64_t px = ox + (int64_t)lat * i, py = oy + (int64_t)lat * j;
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
  const int64_t x = ox + (int64_t)lat * li, y = oy + (int64_t)lat * lj;  // >= 0
  if (x >= (int64_t)w || y >= (int64_t)h) return;
  const uint32_t ce = lj * lw + li;
  const uint32_t key = Guided ? sk[ce] : 0u;
  AtrousCentre p = atrous_centre(sc[ce], Guided ? sg[ce] : float4{}, key, Guided, kc, kn, sigma_depth, (float)s);
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int64_t qy = y + (int64_t)s * dy;
    if (qy < 0 || qy >= (int64_t)h) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int64_t qx = x + (int64_t)s * dx;
      if (qx < 0 || qx >= (int64_t)w) continue;
      const uint32_t e = (uint32_t)((int)lj + (int)m * dy) * lw + (uint32_t)((int)li + (int)m * dx);
      if (Guided && sk[e] != key) continue;
      atrous_tap(p, atrous_k(dx) * atrous_k(dy), sc[e], Guided ? sg[e] : float4{});
    }
  }
  atrous_store(out, (size_t)y * w + (size_t)x, p);
}

constexpr size_t kTiledMaxLds = 64u << 10;  // the dynamic LDS a launch may ask for without an attribute

hipError_t launch_denoise_prep(const void* src, bool f32, const hrt_hit* hits, void* c0, void* guide, void* keys,
                               size_t npix, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  if (!src || !c0 || (hits && (!guide || !keys))) return hipErrorInvalidValue;
  const unsigned int grid = (unsigned int)((npix + 255) / 256);
  const float4* hp = reinterpret_cast<const float4*>(hits);
  if (f32)
    denoise_prep<float4><<<grid, 256, 0, stream>>>(static_cast<const float4*>(src), hp, static_cast<float4*>(c0),
                                                   static_cast<float4*>(guide), static_cast<uint32_t*>(keys), npix);
  else
    denoise_prep<uint32_t><<<grid, 256, 0, stream>>>(static_cast<const uint32_t*>(src), hp, static_cast<float4*>(c0),
                                                     static_cast<float4*>(guide), static_cast<uint32_t*>(keys), npix);
  return hipGetLastError();
}

template <bool Guided, typename Out>
static hipError_t atrous_launch(const AtrousPass& p, int form, hipStream_t stream) {
  const float4* cin = static_cast<const float4*>(p.in);
  const float4* gd = static_cast<const float4*>(p.guide);
  const uint32_t* keys = static_cast<const uint32_t*>(p.keys);
  Out* out = static_cast<Out*>(p.out);
  if (form == kAtrousDirect) {
    const dim3 grid((p.w + kTileW - 1) / kTileW, (p.h + kTileH - 1) / kTileH, 1);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    atrous_direct<Guided, Out><<<grid, 256, 0, stream>>>(cin, gd, keys, out, p.w, p.h, p.step, p.kc, p.kn, p.sigma_depth);
    return hipGetLastError();
  }
  const uint32_t lat = form == kAtrousLattice ? p.step : 1u;
  const uint32_t r = 2u * (p.step / lat);
  const size_t n = (size_t)(kTileW + 2u * r) * (kTileH + 2u * r);
  const size_t bytes = n * (Guided ? 36u : 16u);
  if (bytes > kTiledMaxLds) return hipErrorInvalidValue;
  // per axis: lat residues x the tiles of the longest residue class (ceil(w / lat) lattice points)
  const uint64_t gx = (uint64_t)lat * (((p.w + lat - 1) / lat + kTileW - 1) / kTileW);
  const uint64_t gy = (uint64_t)lat * (((p.h + lat - 1) / lat + kTileH - 1) / kTileH);
  if (gx > 0x7FFFFFFFull || gy > 65535ull) return hipErrorInvalidValue;
  atrous_tiled<Guided, Out><<<dim3((uint32_t)gx, (uint32_t)gy, 1), 256, bytes, stream>>>(cin, gd, keys, out, p.w, p.h, p.step,
                                                                                       lat, p.kc, p.kn, p.sigma_depth);
  return hipGetLastError();
}

hipError_t launch_atrous(const AtrousPass& p, int form, hipStream_t stream) {
  if (p.w == 0 || p.h == 0) return hipSuccess;
  if (!p.in || !p.out || p.in == p.out || (p.guide == nullptr) != (p.keys == nullptr)) return hipErrorInvalidValue;
  if (p.step == 0 || p.step > (1u << (kDenoiseMaxIterations - 1)) || (p.step & (p.step - 1u)) != 0) return hipErrorInvalidValue;
  if (form != kAtrousDirect && form != kAtrousDense && form != kAtrousLattice) return hipErrorInvalidValue;
  if (p.guide)
    return p.out_rgba8 ? atrous_launch<true, uint32_t>(p, form, stream) : atrous_launch<true, float4>(p, form, stream);
  return p.out_rgba8 ? atrous_launch<false, uint32_t>(p, form, stream) : atrous_launch<false, float4>(p, form, stream);
}

}  // namespace hrt
