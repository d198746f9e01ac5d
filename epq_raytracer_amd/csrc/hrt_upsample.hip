// hrt_upsample.hip -- gfx950 kernel of the guided upsample (hrt_upsample.h): one kernel
// family, upsample<Footprint, Out>, a lane per target pixel.
//
// S19 is pinned operation by operation and the unit is built with -ffp-contract=off: every statement of
// upsample_tap and of the store below is one rounded float operation of the spec, in its order; the coordinate
// arithmetic is hrt_upsample_map.h's, which a CPU program checks against the numpy restatement.
#include <hip/hip_runtime.h>

#include "hip_raytrace.h"
#include "hrt_math.h"
#include "hrt_upsample.h"
#include "hrt_upsample_map.h"

namespace hrt {

namespace {

constexpr uint32_t kUpTileW = 32, kUpTileH = 8;  // one pixel per thread of a 256-thread workgroup, a wave = 2 rows

// S14's surface key of a hit record's first 16 bytes {t, kind, index, mesh}.
__device__ __forceinline__ uint32_t upsample_key(uint32_t kind, uint32_t index, uint32_t mesh) {
  if (kind == 1u) return 0x80000000u | (index & 0x7FFFFFFFu);
  if (kind == 2u) return (mesh + 1u) & 0x7FFFFFFFu;
  return 0u;
}

// hrt_present's byte order of an RGBA8 word: bytes 0 and 2 swapped for B8G8R8A8.
__device__ __forceinline__ uint32_t upsample_word(uint32_t v, uint32_t bgra) {
  return bgra ? __builtin_amdgcn_perm(v, v, 0x03000102u) : v;
}

}  // namespace

template <int Footprint, int Out>
__global__ __launch_bounds__(256) void upsample(const float4* __restrict__ low, const float4* __restrict__ guide,
                                                const uint32_t* __restrict__ keys, const float4* __restrict__ high,
                                                void* __restrict__ out, uint32_t ws, uint32_t hs, uint32_t wt,
                                                uint32_t ht, uint32_t pitch, uint32_t bgra, float kn,
                                                float sigma_depth) {
  const uint32_t x = blockIdx.x * kUpTileW + (threadIdx.x & (kUpTileW - 1u));
  const uint32_t y = blockIdx.y * kUpTileH + threadIdx.x / kUpTileW;
  if (x >= wt || y >= ht) return;
  const size_t i = (size_t)y * wt + x;
  const float4 ha = high[2 * i], hb = high[2 * i + 1];  // {t, kind, index, mesh}, {n.x, n.y, n.z, reserved}
  const uint32_t kp = upsample_key(__float_as_uint(ha.y), __float_as_uint(ha.z), __float_as_uint(ha.w));
  const bool weigh = kp != 0u;
  const float tp = ha.x;
  const float kd = weigh ? 1.0f / (sigma_depth * tp) : 0.0f;
  constexpr float inv_r = upsample_inv_r(Footprint);
  const float u = upsample_coord(x, ws, wt), v = upsample_coord(y, hs, ht);
  const float x0 = upsample_first(u), y0 = upsample_first(v);
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int ey = upsample_tap_lo(Footprint); ey <= upsample_tap_hi(Footprint); ++ey) {
    const float yj = y0 + (float)ey;
    if (!upsample_inside(yj, hs)) continue;
    const float wy = upsample_weight(v, yj, inv_r);
    if (!(wy > 0.0f)) continue;
    const size_t row = (size_t)(uint32_t)yj * ws;
#pragma unroll
    for (int ex = upsample_tap_lo(Footprint); ex <= upsample_tap_hi(Footprint); ++ex) {
      const float xj = x0 + (float)ex;
      if (!upsample_inside(xj, ws)) continue;
      const float wx = upsample_weight(u, xj, inv_r);
      if (!(wx > 0.0f)) continue;
      const size_t q = row + (uint32_t)xj;
      if (keys[q] != kp) continue;
      const float h = wx * wy;
      float wn = 1.0f, wd = 1.0f;
      if (weigh) {
        const float4 gq = guide[q];
        const float dot = (hb.x * gq.x + hb.y * gq.y) + hb.z * gq.z;
        const float a = 1.0f - (1.0f - dot) * kn;
        wn = a > 0.0f ? a : 0.0f;
        const float b = 1.0f - fabsf(tp - gq.w) * kd;
        wd = b > 0.0f ? b : 0.0f;
      }
      const float w = (h * wn) * wd;
      const float4 cq = low[q];
      ar = ar + w * cq.x;
      ag = ag + w * cq.y;
      ab = ab + w * cq.z;
      wsum = wsum + w;
    }
  }
  float r, g, b;
  if (wsum > 0.0f) {
    r = ar / wsum;
    g = ag / wsum;
    b = ab / wsum;
  } else {  // no tap kept, every weight 0, or a NaN: the nearest texel
    const float4 c = low[(size_t)upsample_nearest(y, hs, ht) * ws + upsample_nearest(x, ws, wt)];
    r = c.x;
    g = c.y;
    b = c.z;
  }
  if constexpr (Out == kUpsampleOutFloat) {
    static_cast<float4*>(out)[i] = make_float4(r, g, b, 1.0f);
  } else {
    const uint32_t word = unorm8(r) | (unorm8(g) << 8) | (unorm8(b) << 16) | (255u << 24);
    if constexpr (Out == kUpsampleOutRgba8)
      static_cast<uint32_t*>(out)[i] = word;
    else
      reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(out) + (size_t)(ht - 1u - y) * pitch)[x] =
          upsample_word(word, bgra);
  }
}

template <int Footprint, int Out>
static hipError_t upsample_launch(const UpsamplePass& p, hipStream_t stream) {
  const dim3 grid((p.wt + kUpTileW - 1) / kUpTileW, (p.ht + kUpTileH - 1) / kUpTileH, 1);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  upsample<Footprint, Out><<<grid, 256, 0, stream>>>(
      static_cast<const float4*>(p.low), static_cast<const float4*>(p.guide), static_cast<const uint32_t*>(p.keys),
      reinterpret_cast<const float4*>(p.high), p.out, p.ws, p.hs, p.wt, p.ht, p.pitch, p.bgra, p.kn, p.sigma_depth);
  return hipGetLastError();
}

template <int Footprint>
static hipError_t upsample_launch_out(const UpsamplePass& p, hipStream_t stream) {
  switch (p.out_kind) {
    case kUpsampleOutFloat: return upsample_launch<Footprint, kUpsampleOutFloat>(p, stream);
    case kUpsampleOutRgba8: return upsample_launch<Footprint, kUpsampleOutRgba8>(p, stream);
    case kUpsampleOutPresent: return upsample_launch<Footprint, kUpsampleOutPresent>(p, stream);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_upsample(const UpsamplePass& p, hipStream_t stream) {
  if (!p.low || !p.guide || !p.keys || !p.high || !p.out) return hipErrorInvalidValue;
  if (p.ws == 0 || p.hs == 0 || p.wt == 0 || p.ht == 0 || p.wt > 16384u || p.ht > 16384u) return hipErrorInvalidValue;
  if (p.ws > (1u << 24) || p.hs > (1u << 24)) return hipErrorInvalidValue;  // float(ws - 1) must be exact
  if (p.out_kind == kUpsampleOutPresent && (p.pitch % 4 != 0 || p.pitch / 4 < p.wt)) return hipErrorInvalidValue;
  if (p.footprint == 2) return upsample_launch_out<2>(p, stream);
  if (p.footprint == 4) return upsample_launch_out<4>(p, stream);
  return hipErrorInvalidValue;
}

}  // namespace hrt
