// hrt_refine.hip -- gfx950 kernels of the adaptive refinement (hrt_refine.h):
// refine_select, which marks the pixels whose pooled standard error is still above the tolerance; refine_queries,
// which turns a mask into a compact list of radiance queries; refine_fold, which folds the queries' results into
// their pixels; and refine_fold_image, the masked fold of a whole traced frame.
//
// S17 is pinned operation by operation and the unit is built with -ffp-contract=off: every statement of the
// selection below is one rounded float operation of the spec, in its order; '/' is the correctly rounded one
// (S4) and a comparison with a NaN is false.  The folds are hrt_history_fold.h's device functions, the ones
// fold_history[_moments] run: a refined pixel gets hrt_accumulate_history[_moments]'s bytes by construction.
//
// Wave primitives: a wave owns 64 consecutive pixels (256-thread workgroups, pixel = global thread index), so
// its 64-bit __ballot is exactly the two mask words of those pixels, and one lane adds the wave's popcount to a
// counter with one integer atomic; refine_queries takes its slots from that atomic's return value plus the
// lane's rank among the set bits below it (mbcnt).  No lane leaves before its wave's ballot.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hip_raytrace.h"
#include "hrt_history.h"
#include "hrt_history_fold.h"
#include "hrt_math.h"
#include "hrt_plan.h"
#include "hrt_refine.h"
#include "hrt_refine_tile_bits.h"

namespace hrt {

// The rank of this lane among the set bits of `bits` below it.
__device__ __forceinline__ uint32_t lane_rank(unsigned long long bits) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(bits >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bits, 0u));
}

// ---- the selection (S17) -----------------------------------------------------------------------------------
// One pixel per lane, the direct form: a tap is 12 bytes (count and moments) and, guided, the first 16 bytes of
// its hit record.  Neighbouring lanes read neighbouring taps, so a row of the window is one run of cache lines.
template <bool Guided>
__global__ __launch_bounds__(256) void refine_select(const uint32_t* __restrict__ cnt, const float2* __restrict__ mom,
                                                     const float4* __restrict__ hits, uint32_t* __restrict__ mask,
                                                     unsigned long long* __restrict__ selected, uint32_t w, uint32_t h,
                                                     RefineRuleK r) {
  const uint32_t npix = w * h;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool sel = false;
  if (i < npix) {
    const uint32_t n = cnt[i];
    if (n >= r.max_count) {
      sel = false;
    } else if (n < r.min_history) {
      sel = true;
    } else {
      const int x = (int)(i % w), y = (int)(i / w);
      const int rad = (int)r.radius;
      uint32_t kp = 0u;
      if constexpr (Guided) kp = hist_key(hits[2 * (size_t)i]);
      float pv = 0.0f, pm = 0.0f, k = 0.0f;
      for (int dy = -rad; dy <= rad; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)h) continue;
        for (int dx = -rad; dx <= rad; ++dx) {
          const int qx = x + dx;
          if (qx < 0 || qx >= (int)w) continue;
          const size_t q = (size_t)qy * w + (size_t)qx;
          if constexpr (Guided) {
            if (hist_key(hits[2 * q]) != kp) continue;
          }
          const uint32_t nq = cnt[q];
          if (nq < r.min_history) continue;
          const float2 m = mom[q];
          const float d = m.y - m.x * m.x;
          const float tv = d > 0.0f ? d : 0.0f;
          pv = pv + tv / (float)nq;
          pm = pm + m.x;
          k = k + 1.0f;
        }
      }
      const float a = pv / k, b = pm / k;
      const float mu = b > r.luminance_floor ? b : r.luminance_floor;
      sel = a > r.tol2 * (mu * mu);
    }
  }
  const unsigned long long bits = __ballot(sel);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t base = i - lane;  // the wave's first pixel: a multiple of 64
  if (lane == 0u && base < npix) {
    mask[base >> 5] = (uint32_t)bits;
    const uint32_t c = (uint32_t)__popcll(bits);
    if (c) atomicAdd(selected, (unsigned long long)c);
  }
  if (lane == 32u && base + 32u < npix) mask[(base >> 5) + 1u] = (uint32_t)(bits >> 32);
}

// ---- mask -> query list ------------------------------------------------------------------------------------
// Emit false: the count alone (queries, index and rays are not touched).
template <bool Emit>
__global__ __launch_bounds__(256) void refine_queries(const uint32_t* __restrict__ mask, const float4* __restrict__ rays,
                                                      float4* __restrict__ queries, uint32_t* __restrict__ index,
                                                      uint32_t* __restrict__ next, uint32_t npix, float cx, float cy,
                                                      float cz, uint32_t seed_base) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool sel = i < npix && ((mask[i >> 5] >> (i & 31u)) & 1u) != 0u;
  const unsigned long long bits = __ballot(sel);
  if (bits == 0ull) return;  // (the same in every lane)
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t first = 0u;
  if (lane == 0u) first = atomicAdd(next, (uint32_t)__popcll(bits));
  if constexpr (Emit) {
    first = __shfl(first, 0, 64);
    if (sel) {
      const uint32_t slot = first + lane_rank(bits);  // < the mask's set bits <= npix: inside the lists
      const float4 c = rays[i];
      queries[2 * (size_t)slot] = make_float4(cx, cy, cz, __uint_as_float(seed_base + i));
      queries[2 * (size_t)slot + 1] = make_float4(c.x, c.y, c.z, 0.0f);
      index[slot] = i;
    }
  }
}

// ---- the folds ---------------------------------------------------------------------------------------------
// The texel hrt_trace stores for a radiance result in the context's mode (RGBA8: S7's store, alpha 255).
template <typename T>
__device__ __forceinline__ T refine_texel(float4 v) {
  if constexpr (std::is_same_v<T, uint32_t>)
    return unorm8(v.x) | (unorm8(v.y) << 8) | (unorm8(v.z) << 16) | (255u << 24);
  else
    return v;
}
template <typename T>
__device__ __forceinline__ T texel_zero() {
  if constexpr (std::is_same_v<T, uint32_t>)
    return 0u;
  else
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
// fold_history[_moments]'s per-pixel statements for pixel p and trace texel v.
template <typename T, bool Moments>
__device__ __forceinline__ void refine_fold_pixel(T* cur, uint32_t* cnt, float2* mom, size_t p, T v, uint32_t max_history,
                                                  const float* tab) {
  const uint32_t n = cnt[p];
  cur[p] = hist_step(n == 0u ? texel_zero<T>() : cur[p], v, n, tab);
  cnt[p] = hist_next(n, max_history);
  if constexpr (Moments) mom[p] = moments_step(n == 0u ? make_float2(0.0f, 0.0f) : mom[p], v, n, tab);
}
// The workgroup's UNORM8 table of the RGBA8 folds (fold_history's), nullptr in float mode.
template <typename T>
__device__ __forceinline__ const float* fold_table(float* tab) {
  if constexpr (std::is_same_v<T, uint32_t>) {
    tab[threadIdx.x] = unorm8_to_float(threadIdx.x);
    __syncthreads();
    return tab;
  } else {
    return nullptr;
  }
}

// One lane per list entry; the entries' pixels are distinct, so no two lanes touch one pixel.
template <typename T, bool Moments>
__global__ __launch_bounds__(256) void refine_fold(T* cur, uint32_t* cnt, float2* mom, const float4* __restrict__ rgba,
                                                   const uint32_t* __restrict__ index, uint32_t n, uint32_t max_history) {
  __shared__ float tab_s[std::is_same_v<T, uint32_t> ? 256 : 1];
  const float* tab = fold_table<T>(tab_s);
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  refine_fold_pixel<T, Moments>(cur, cnt, mom, index[e], refine_texel<T>(rgba[e]), max_history, tab);
}

// One lane per pixel of the image; a lane whose bit is clear touches nothing.
template <typename T, bool Moments>
__global__ __launch_bounds__(256) void refine_fold_image(T* cur, const T* __restrict__ nw, uint32_t* cnt, float2* mom,
                                                         const uint32_t* __restrict__ mask, uint32_t npix,
                                                         uint32_t max_history) {
  __shared__ float tab_s[std::is_same_v<T, uint32_t> ? 256 : 1];
  const float* tab = fold_table<T>(tab_s);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= npix || ((mask[i >> 5] >> (i & 31u)) & 1u) == 0u) return;
  refine_fold_pixel<T, Moments>(cur, cnt, mom, i, nw[i], max_history, tab);
}

// ---- the tile-masked pass (hrt_refine_tiles) --------------------------------------------
// Pixel mask -> one bit per 8x8 tile: one lane per tile, so a wave's ballot is the two bit words of its 64 tiles
// (each written in full).  counts (zeroed by the caller) += {the set bits of real pixels, the selected tiles, the
// real pixels of the selected tiles}.
__global__ __launch_bounds__(256) void refine_tile_bits(const uint32_t* __restrict__ mask, uint32_t* __restrict__ bits,
                                                        unsigned long long* __restrict__ counts, uint32_t w, uint32_t h) {
  const uint32_t tiles_x = (w + 7u) / 8u, tiles = tiles_x * ((h + 7u) / 8u);
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  uint32_t sel = 0u, real = 0u;
  if (t < tiles) {
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    sel = tile_selected_pixels(mask, w, h, tx, ty, &real);
  }
  const unsigned long long on = __ballot(sel != 0u);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t base = t - lane;  // the wave's first tile: a multiple of 64
  if (lane == 0u && base < tiles) bits[base >> 5] = (uint32_t)on;
  if (lane == 32u && base + 32u < tiles) bits[(base >> 5) + 1u] = (uint32_t)(on >> 32);
  if (on == 0ull) return;  // (the same in every lane)
  uint32_t traced = sel != 0u ? real : 0u;  // (a wave's sums are at most 64 x 64)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sel += __shfl_xor(sel, off, 64);
    traced += __shfl_xor(traced, off, 64);
  }
  if (lane == 0u) {
    atomicAdd(&counts[0], (unsigned long long)sel);
    atomicAdd(&counts[1], (unsigned long long)__popcll(on));
    atomicAdd(&counts[2], (unsigned long long)traced);
  }
}

// plan_hist / plan_fill (hrt_kernels.hip) over the tiles whose bit is set: the same buckets, sky rule, heavy
// split, priority flag and item words (hrt_plan.h), with the tile's input cost from `cost`, or 1 for every tile
// when cost is null.  The histogram pass also sums the selected tiles' input costs into sched[6..7], the u64 a
// whole frame's trace leaves there and plan_scan reads (zeroed by the caller).
__device__ __forceinline__ bool tile_bit(const uint32_t* bits, uint32_t t) { return ((bits[t >> 5] >> (t & 31u)) & 1u) != 0u; }
__global__ __launch_bounds__(256) void plan_hist_masked(uint32_t* sched, const uint32_t* __restrict__ cost,
                                                        const uint32_t* __restrict__ bits, uint32_t tiles,
                                                        const uint32_t* tl_cache) {
  __shared__ uint32_t h[kPlanBuckets];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (threadIdx.x < kPlanBuckets) h[threadIdx.x] = 0;
  __syncthreads();
  const bool sel = i < tiles && tile_bit(bits, i);
  unsigned long long c = 0ull;
  if (sel) {
    const uint32_t ci = cost ? cost[i] : 1u;
    atomicAdd(&h[plan_bucket_of(ci, tl_cache, i)], 1u);
    c = ci;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63u) == 0u && c) atomicAdd(reinterpret_cast<unsigned long long*>(sched + 6), c);
  __syncthreads();
  if (threadIdx.x < kPlanBuckets && h[threadIdx.x]) atomicAdd(&sched[kSchedHist + threadIdx.x], h[threadIdx.x]);
}
__global__ __launch_bounds__(256) void plan_fill_masked(uint32_t* sched, const uint32_t* __restrict__ cost,
                                                        const uint32_t* __restrict__ bits, uint32_t tiles, uint32_t kmax,
                                                        uint32_t prio, uint32_t* items, const uint32_t* tl_cache) {
  __shared__ uint32_t cnt[kPlanBuckets], base[kPlanBuckets];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (threadIdx.x < kPlanBuckets) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t hb = sched[3];
  const bool sel = i < tiles && tile_bit(bits, i);
  const uint32_t b = sel ? plan_bucket_of(cost ? cost[i] : 1u, tl_cache, i) : 0u;
  const bool heavy = b >= hb;
  const uint32_t k = bucket_items(b, hb, kmax);
  const uint32_t local = sel ? atomicAdd(&cnt[b], k) : 0u;
  __syncthreads();
  if (threadIdx.x < kPlanBuckets && cnt[threadIdx.x])
    base[threadIdx.x] = sched[kSchedOff + threadIdx.x] + atomicAdd(&sched[kSchedCur + threadIdx.x], cnt[threadIdx.x]);
  __syncthreads();
  if (!sel) return;
  const uint32_t at = base[b] + local;  // < the plan's items <= 64 x the selected tiles: inside the item list
  if (!heavy) {
    items[at] = i;
  } else {
    const uint32_t flag = prio ? 0x80000000u : 0u;
    if (k == 1) {
      items[at] = i | flag;
    } else {
      const uint32_t lk = (uint32_t)__builtin_ctz(k);
      for (uint32_t s = 0; s < k; ++s) items[at + s] = i | (lk << 22) | (s << 25) | flag;
    }
  }
}

// One lane per pixel.  A pixel whose bit is set folds the launch's nf frames (frame f's texel at stack[f stride +
// i]) in order, in registers -- refine_fold_pixel's statements nf times -- and stores A, N and M once; nf = 1 is
// refine_fold_image.  trace (null: the stack is the trace image already) gets the last frame's texel of every
// pixel whose tile's bit is set; no other byte of it is touched.
template <typename T, bool Moments>
__global__ __launch_bounds__(256) void refine_fold_frames(T* cur, const T* __restrict__ stack, size_t stride, uint32_t nf,
                                                          uint32_t* cnt, float2* mom, const uint32_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ tile_bits, T* __restrict__ trace,
                                                          uint32_t w, uint32_t npix, uint32_t max_history) {
  __shared__ float tab_s[std::is_same_v<T, uint32_t> ? 256 : 1];
  const float* tab = fold_table<T>(tab_s);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= npix) return;
  const bool sel = ((mask[i >> 5] >> (i & 31u)) & 1u) != 0u;
  bool copy = false;
  if (trace) {
    const uint32_t y = i / w, x = i - y * w;
    copy = tile_bit(tile_bits, (x >> 3) + (y >> 3) * ((w + 7u) / 8u));
  }
  if (!sel && !copy) return;
  T v;
  if (sel) {
    uint32_t n = cnt[i];
    T a = n == 0u ? texel_zero<T>() : cur[i];
    float2 m = make_float2(0.0f, 0.0f);
    if constexpr (Moments) {
      if (n != 0u) m = mom[i];
    }
    for (uint32_t f = 0; f < nf; ++f) {
      v = stack[(size_t)f * stride + i];
      a = hist_step(a, v, n, tab);
      if constexpr (Moments) m = moments_step(m, v, n, tab);
      n = hist_next(n, max_history);
    }
    cur[i] = a;
    cnt[i] = n;
    if constexpr (Moments) mom[i] = m;
  } else {
    v = stack[(size_t)(nf - 1u) * stride + i];
  }
  if (copy) trace[i] = v;
}

// ---- launch wrappers (host) ----------------------------------------------------------------------------------
static uint32_t blocks_of(uint32_t n) { return (uint32_t)(((uint64_t)n + 255u) / 256u); }

hipError_t launch_refine_select(const uint32_t* cnt, const float* mom, const hrt_hit* hits, uint32_t* mask,
                                unsigned long long* selected, uint32_t w, uint32_t h, const RefineRuleK& rule,
                                hipStream_t stream) {
  if (w == 0 || h == 0) return hipSuccess;
  if (!cnt || !mom || !mask || !selected || (uint64_t)w * h > 0x80000000ull) return hipErrorInvalidValue;
  if (((uintptr_t)mom & 7u) != 0 || ((uintptr_t)mask & 3u) != 0 || ((uintptr_t)hits & 15u) != 0) return hipErrorInvalidValue;
  if (rule.radius > 3u || rule.min_history == 0u || rule.max_count < rule.min_history) return hipErrorInvalidValue;
  const float2* m = reinterpret_cast<const float2*>(mom);
  const uint32_t blocks = blocks_of(w * h);
  if (hits)
    refine_select<true><<<blocks, 256, 0, stream>>>(cnt, m, reinterpret_cast<const float4*>(hits), mask, selected, w, h, rule);
  else
    refine_select<false><<<blocks, 256, 0, stream>>>(cnt, m, nullptr, mask, selected, w, h, rule);
  return hipGetLastError();
}

hipError_t launch_refine_queries(const uint32_t* mask, const float4* rays, float4* queries, uint32_t* index,
                                 uint32_t* next, uint32_t npix, const float cam_pos[3], uint32_t seed_base,
                                 hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  if (!mask || !next || ((uintptr_t)mask & 3u) != 0) return hipErrorInvalidValue;
  if (queries) {
    if (!rays || !index || ((uintptr_t)queries & 15u) != 0 || !cam_pos) return hipErrorInvalidValue;
    refine_queries<true><<<blocks_of(npix), 256, 0, stream>>>(mask, rays, queries, index, next, npix, cam_pos[0], cam_pos[1],
                                                             cam_pos[2], seed_base);
  } else {
    refine_queries<false><<<blocks_of(npix), 256, 0, stream>>>(mask, nullptr, nullptr, nullptr, next, npix, 0.0f, 0.0f, 0.0f,
                                                              0u);
  }
  return hipGetLastError();
}

static bool fold_args_ok(const void* cur, const uint32_t* cnt, const float* mom, bool f32, uint32_t max_history) {
  if (!cur || !cnt || max_history == 0 || max_history > kHistoryMax) return false;
  if (f32 && ((uintptr_t)cur & 15u) != 0) return false;
  return ((uintptr_t)mom & 7u) == 0;
}

hipError_t launch_refine_fold(void* cur, uint32_t* cnt, float* mom, bool f32, const float4* rgba, const uint32_t* index,
                              uint32_t n, uint32_t max_history, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!fold_args_ok(cur, cnt, mom, f32, max_history) || !rgba || !index || ((uintptr_t)rgba & 15u) != 0)
    return hipErrorInvalidValue;
  float2* m = reinterpret_cast<float2*>(mom);
  const uint32_t blocks = blocks_of(n);
  if (f32) {
    float4* c = static_cast<float4*>(cur);
    if (mom)
      refine_fold<float4, true><<<blocks, 256, 0, stream>>>(c, cnt, m, rgba, index, n, max_history);
    else
      refine_fold<float4, false><<<blocks, 256, 0, stream>>>(c, cnt, nullptr, rgba, index, n, max_history);
  } else {
    uint32_t* c = static_cast<uint32_t*>(cur);
    if (mom)
      refine_fold<uint32_t, true><<<blocks, 256, 0, stream>>>(c, cnt, m, rgba, index, n, max_history);
    else
      refine_fold<uint32_t, false><<<blocks, 256, 0, stream>>>(c, cnt, nullptr, rgba, index, n, max_history);
  }
  return hipGetLastError();
}

hipError_t launch_refine_fold_image(void* cur, const void* nw, uint32_t* cnt, float* mom, bool f32, const uint32_t* mask,
                                    uint32_t npix, uint32_t max_history, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  if (!fold_args_ok(cur, cnt, mom, f32, max_history) || !nw || !mask || ((uintptr_t)mask & 3u) != 0)
    return hipErrorInvalidValue;
  if (f32 && ((uintptr_t)nw & 15u) != 0) return hipErrorInvalidValue;
  float2* m = reinterpret_cast<float2*>(mom);
  const uint32_t blocks = blocks_of(npix);
  if (f32) {
    float4* c = static_cast<float4*>(cur);
    const float4* v = static_cast<const float4*>(nw);
    if (mom)
      refine_fold_image<float4, true><<<blocks, 256, 0, stream>>>(c, v, cnt, m, mask, npix, max_history);
    else
      refine_fold_image<float4, false><<<blocks, 256, 0, stream>>>(c, v, cnt, nullptr, mask, npix, max_history);
  } else {
    uint32_t* c = static_cast<uint32_t*>(cur);
    const uint32_t* v = static_cast<const uint32_t*>(nw);
    if (mom)
      refine_fold_image<uint32_t, true><<<blocks, 256, 0, stream>>>(c, v, cnt, m, mask, npix, max_history);
    else
      refine_fold_image<uint32_t, false><<<blocks, 256, 0, stream>>>(c, v, cnt, nullptr, mask, npix, max_history);
  }
  return hipGetLastError();
}

hipError_t launch_refine_tile_bits(const uint32_t* mask, uint32_t* bits, unsigned long long* counts, uint32_t w, uint32_t h,
                                   hipStream_t stream) {
  if (w == 0 || h == 0) return hipSuccess;
  if (!mask || !bits || !counts || ((uintptr_t)mask & 3u) != 0 || (uint64_t)w * h > 0x80000000ull) return hipErrorInvalidValue;
  const uint32_t tiles = ((w + 7u) / 8u) * ((h + 7u) / 8u);
  refine_tile_bits<<<blocks_of(tiles), 256, 0, stream>>>(mask, bits, counts, w, h);
  return hipGetLastError();
}

hipError_t launch_plan_hist_masked(uint32_t* sched, const uint32_t* cost, const uint32_t* bits, uint32_t tiles,
                                   const uint32_t* tl_cache, hipStream_t stream) {
  if (!sched || !bits || tiles == 0 || tiles > kItemTileMask) return hipErrorInvalidValue;
  plan_hist_masked<<<blocks_of(tiles), 256, 0, stream>>>(sched, cost, bits, tiles, tl_cache);
  return hipGetLastError();
}

hipError_t launch_plan_fill_masked(uint32_t* sched, const uint32_t* cost, const uint32_t* bits, uint32_t tiles, uint32_t kmax,
                                   uint32_t prio, uint32_t* items, const uint32_t* tl_cache, hipStream_t stream) {
  if (!sched || !bits || !items || tiles == 0 || tiles > kItemTileMask || kmax == 0 || kmax > 64u) return hipErrorInvalidValue;
  plan_fill_masked<<<blocks_of(tiles), 256, 0, stream>>>(sched, cost, bits, tiles, kmax, prio, items, tl_cache);
  return hipGetLastError();
}

hipError_t launch_refine_fold_frames(void* cur, const void* stack, size_t stride, uint32_t nf, uint32_t* cnt, float* mom,
                                     bool f32, const uint32_t* mask, const uint32_t* tile_bits, void* trace, uint32_t w,
                                     uint32_t h, uint32_t max_history, hipStream_t stream) {
  if (w == 0 || h == 0 || nf == 0) return hipSuccess;
  if (!fold_args_ok(cur, cnt, mom, f32, max_history) || !stack || !mask || ((uintptr_t)mask & 3u) != 0 ||
      (uint64_t)w * h > 0x80000000ull || (trace && !tile_bits) || (nf > 1 && stride < (size_t)w * h))
    return hipErrorInvalidValue;
  if (f32 && ((((uintptr_t)stack | (uintptr_t)trace) & 15u) != 0)) return hipErrorInvalidValue;
  float2* m = reinterpret_cast<float2*>(mom);
  const uint32_t npix = w * h, blocks = blocks_of(npix);
  if (f32) {
    float4* c = static_cast<float4*>(cur);
    const float4* s = static_cast<const float4*>(stack);
    float4* t = static_cast<float4*>(trace);
    if (mom)
      refine_fold_frames<float4, true><<<blocks, 256, 0, stream>>>(c, s, stride, nf, cnt, m, mask, tile_bits, t, w, npix, max_history);
    else
      refine_fold_frames<float4, false><<<blocks, 256, 0, stream>>>(c, s, stride, nf, cnt, nullptr, mask, tile_bits, t, w, npix,
                                                                    max_history);
  } else {
    uint32_t* c = static_cast<uint32_t*>(cur);
    const uint32_t* s = static_cast<const uint32_t*>(stack);
    uint32_t* t = static_cast<uint32_t*>(trace);
    if (mom)
      refine_fold_frames<uint32_t, true><<<blocks, 256, 0, stream>>>(c, s, stride, nf, cnt, m, mask, tile_bits, t, w, npix, max_history);
    else
      refine_fold_frames<uint32_t, false><<<blocks, 256, 0, stream>>>(c, s, stride, nf, cnt, nullptr, mask, tile_bits, t, w, npix,
                                                                      max_history);
  }
  return hipGetLastError();
}

}  // namespace hrt
