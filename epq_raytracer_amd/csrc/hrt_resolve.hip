// hrt_resolve.hip -- gfx950 kernel of the fold across resolutions (hrt_resolve.h): one
// kernel family, resolve<T, Moments, Guided>, a lane per target pixel.
//
// S20 is pinned operation by operation and the unit is built with -ffp-contract=off: the coordinate arithmetic is
// hrt_resolve_map.h's, which a CPU program checks against the numpy restatement, and an accepted pixel's step is
// hrt_history_fold.h's, the one fold_history[_moments] takes.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hip_raytrace.h"
#include "hrt_history.h"
#include "hrt_history_fold.h"
#include "hrt_math.h"
#include "hrt_resolve.h"
#include "hrt_resolve_map.h"

namespace hrt {

namespace {

constexpr uint32_t kRsTileW = 32, kRsTileH = 8;  // one pixel per thread of a 256-thread workgroup, a wave = 2 rows

}  // namespace

// A wave's 2 x 32 target pixels map to at most two source rows (one when the source is the smaller image), so
// its texel and hit-record reads share cache lines; a pixel that is not accepted and not filled reads its count
// (and, guided, nothing else) and writes nothing.
template <typename T, bool Moments, bool Guided>
__global__ __launch_bounds__(256) void resolve(T* __restrict__ acc, uint32_t* __restrict__ cnt, float2* __restrict__ mom,
                                               const T* __restrict__ src, const float4* __restrict__ src_hits,
                                               const float4* __restrict__ hits, uint32_t ws, uint32_t hs, uint32_t w,
                                               uint32_t h, float ox, float oy, uint32_t max_history, uint32_t fill) {
  const float* tab = nullptr;
  if constexpr (std::is_same_v<T, uint32_t>) {
    __shared__ float table[256];
    table[threadIdx.x] = unorm8_to_float(threadIdx.x);
    __syncthreads();
    tab = table;
  }
  const uint32_t x = blockIdx.x * kRsTileW + (threadIdx.x & (kRsTileW - 1u));
  const uint32_t y = blockIdx.y * kRsTileH + threadIdx.x / kRsTileW;
  if (x >= w || y >= h) return;
  const size_t p = (size_t)y * w + x;
  const float u = resolve_coord(x, ws, w, ox), v = resolve_coord(y, hs, h, oy);
  const float i = resolve_sample(u), j = resolve_sample(v);
  bool accepted = resolve_inside(i, ws) && resolve_inside(j, hs) && resolve_own(resolve_dist(u, i), ws, w) &&
                  resolve_own(resolve_dist(v, j), hs, h);
  if constexpr (Guided) {
    if (accepted) {  // (inside: the conversions are defined)
      const size_t q = (size_t)(uint32_t)j * ws + (uint32_t)i;
      accepted = hist_key(src_hits[2 * q]) == hist_key(hits[2 * p]);
    }
  }
  const uint32_t n = cnt[p];
  if (accepted) {
    const T t = src[(size_t)(uint32_t)j * ws + (uint32_t)i];
    if constexpr (std::is_same_v<T, uint32_t>)
      acc[p] = hist_step(n == 0u ? 0u : acc[p], t, n, tab);
    else
      acc[p] = hist_step(n == 0u ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : acc[p], t, n, tab);
    if constexpr (Moments) mom[p] = moments_step(n == 0u ? make_float2(0.0f, 0.0f) : mom[p], t, n, tab);
    cnt[p] = hist_next(n, max_history);
  } else if (fill != 0u && n == 0u) {
    const float ic = resolve_clamp(i, ws), jc = resolve_clamp(j, hs);
    acc[p] = hist_first(src[(size_t)(uint32_t)jc * ws + (uint32_t)ic]);
  }
}

template <typename T, bool Moments, bool Guided>
static void resolve_launch(const ResolvePass& p, dim3 grid, hipStream_t stream) {
  resolve<T, Moments, Guided><<<grid, 256, 0, stream>>>(
      static_cast<T*>(p.acc), p.cnt, reinterpret_cast<float2*>(p.mom), static_cast<const T*>(p.src),
      reinterpret_cast<const float4*>(p.src_hits), reinterpret_cast<const float4*>(p.hits), p.ws, p.hs, p.w, p.h,
      p.offset_x, p.offset_y, p.max_history, p.fill);
}

template <typename T>
static void resolve_launch_form(const ResolvePass& p, dim3 grid, hipStream_t stream) {
  const bool guided = p.hits != nullptr;
  if (p.mom) {
    if (guided)
      resolve_launch<T, true, true>(p, grid, stream);
    else
      resolve_launch<T, true, false>(p, grid, stream);
  } else if (guided) {
    resolve_launch<T, false, true>(p, grid, stream);
  } else {
    resolve_launch<T, false, false>(p, grid, stream);
  }
}

hipError_t launch_resolve(const ResolvePass& p, hipStream_t stream) {
  if (!p.acc || !p.cnt || !p.src) return hipErrorInvalidValue;
  if ((p.src_hits == nullptr) != (p.hits == nullptr)) return hipErrorInvalidValue;
  if (p.ws == 0 || p.hs == 0 || p.w == 0 || p.h == 0) return hipErrorInvalidValue;
  // float(ws - 1), float(w) and the pixel coordinates must be exact
  if (p.ws > (1u << 24) || p.hs > (1u << 24) || p.w > (1u << 24) || p.h > (1u << 24)) return hipErrorInvalidValue;
  if (p.max_history == 0 || p.max_history > kHistoryMax) return hipErrorInvalidValue;
  if (!(p.offset_x >= -0.5f && p.offset_x <= 0.5f && p.offset_y >= -0.5f && p.offset_y <= 0.5f)) return hipErrorInvalidValue;
  if (p.f32 && (((uintptr_t)p.acc | (uintptr_t)p.src) & 15u) != 0) return hipErrorInvalidValue;
  if (((uintptr_t)p.mom & 7u) != 0) return hipErrorInvalidValue;
  if ((((uintptr_t)p.src_hits | (uintptr_t)p.hits) & 15u) != 0) return hipErrorInvalidValue;
  const dim3 grid((p.w + kRsTileW - 1) / kRsTileW, (p.h + kRsTileH - 1) / kRsTileH, 1);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  if (p.f32)
    resolve_launch_form<float4>(p, grid, stream);
  else
    resolve_launch_form<uint32_t>(p, grid, stream);
  return hipGetLastError();
}

}  // namespace hrt
