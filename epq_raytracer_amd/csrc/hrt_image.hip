// hrt_image.hip -- gfx950 kernels of the image passes: the init clear, the progressive accumulator
// (assets/image_combiner.glsl) with its fold records, format conversion, the present pass and the
// row-tile assembly, and their launchers (hrt_image.h).  Nothing here is shared with the trace unit
// (hrt_kernels.hip) beyond the device helpers of hrt_math.h and hrt_present_map.h.
//
// One kernel family over the pixel type T: uint32_t (a packed RGBA8 word) or float4 (RGBA32F).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "hip_raytrace.h"
#include "hrt_image.h"
#include "hrt_math.h"
#include "hrt_present_map.h"

namespace hrt {

// The RGBA8 word of a float4 texel: what hrt_read_image's conversion, the present pass and the fold
// records' displayed image show of an RGBA32F pixel.
__device__ __forceinline__ uint32_t pack_rgba8(float4 v) {
  return unorm8(v.x) | (unorm8(v.y) << 8) | (unorm8(v.z) << 16) | (unorm8(v.w) << 24);
}
__device__ __forceinline__ uint32_t displayed_word(uint32_t v) { return v; }
__device__ __forceinline__ uint32_t displayed_word(float4 v) { return pack_rgba8(v); }

// ---- init clear (raytracing.glsl:363-366) and image_combiner.glsl (:22-43) ----------------------
template <typename T>
__global__ __launch_bounds__(256) void clear_kernel(T* img, size_t npix) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix) return;
  if constexpr (std::is_same_v<T, uint32_t>)
    img[i] = 255u << 24;
  else
    img[i] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
}

// image_combiner.glsl:22-43 for one pixel: frame 0 clears, frame k folds the new frame in.
__device__ __forceinline__ float4 combine_rgba32f(float4 p, float4 n, uint32_t frame) {
  if (frame == 0) return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
  const float ff = (float)frame, ff1 = (float)(frame + 1u);
  return make_float4((n.x + p.x * ff) / ff1, (n.y + p.y * ff) / ff1, (n.z + p.z * ff) / ff1, 1.0f);
}
// The RGBA8 combiner with its nine IEEE divisions replaced by the same quotients (r05): the six UNORM8 loads
// k / 255 from a 256-entry table of those quotients (unorm8_to_float, built once per workgroup in LDS),
// and the three divisions by frame + 1 through that denominator's reciprocal, shared by the channels
// (div_core: rcp_core is RN(1 / b) on [2^-40, 2^40], every numerator here is 0 or in [2^-8, 2^33], so
// Markstein's correction gives the correctly rounded quotient; a zero numerator gives +0 as the IEEE
// division does).  The reference spelling is the oracle's (orc_accumulate_rgba8: unorm8((nc + prev * ff) /
// ff1) per channel); tests/test_gpu_parity.py holds every accumulator to it.
// Domain: every uint32_t frame.  ff1 is 0 or in [1, 2^32]: frames 1 .. 2^32 - 2 take the shared reciprocal
// (tests/test_gpu_image_exhaustive.py enumerates all 65,536 channel pairs over frames 0 .. 1199 and the edges
// 2^24 +- 1, 2^31, 2^32 - 3 .. 2^32 - 1 on the device).  At frame 2^32 - 1, frame + 1 wraps to 0 and
// rcp_core(0) = fma(fma(-0, inf, 1), inf, inf) is NaN where the reference divides by zero (+inf, stored as
// 255, for a nonzero numerator; NaN, stored as 0, for 0 / 0): that frame -- any ff1 outside rcp_core's
// range -- takes the IEEE '/' spelling.  The branch is workgroup-uniform (frame is a kernel argument).
__device__ __forceinline__ uint32_t combine_rgba8_fast(uint32_t pv, uint32_t nv, uint32_t frame, const float* tab) {
  if (frame == 0) return 255u << 24;
  const float ff = (float)frame, ff1 = (float)(frame + 1u);
  uint32_t out = 255u << 24;
  if (__builtin_expect(!(ff1 >= 0x1p-40f && ff1 <= 0x1p40f), 0)) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float prev = tab[(pv >> (8 * ch)) & 255u];
      const float nc = tab[(nv >> (8 * ch)) & 255u];
      out |= unorm8((nc + prev * ff) / ff1) << (8 * ch);
    }
    return out;
  }
  const float y = rcp_core(ff1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float prev = tab[(pv >> (8 * ch)) & 255u];
    const float nc = tab[(nv >> (8 * ch)) & 255u];
    out |= unorm8(div_core(nc + prev * ff, ff1, y)) << (8 * ch);
  }
  return out;
}
__device__ __forceinline__ void unorm8_table(float* tab) {  // blockDim.x == 256
  tab[threadIdx.x] = unorm8_to_float(threadIdx.x);
  __syncthreads();
}
// The fold chain's step and its table: only the RGBA8 instantiations keep the UNORM8 table in LDS (and
// its barrier); the RGBA32F ones get a null table that fold_step ignores.
__device__ __forceinline__ uint32_t fold_step(uint32_t v, uint32_t n, uint32_t frame, const float* tab) {
  return combine_rgba8_fast(v, n, frame, tab);
}
__device__ __forceinline__ float4 fold_step(float4 v, float4 n, uint32_t frame, const float*) {
  return combine_rgba32f(v, n, frame);
}
template <typename T>
__device__ __forceinline__ const float* fold_table() {  // every thread of a 256-thread workgroup calls it
  if constexpr (std::is_same_v<T, uint32_t>) {
    __shared__ float tab[256];
    unorm8_table(tab);
    return tab;
  } else {
    return nullptr;
  }
}
template <typename T>
__device__ __forceinline__ T fold_zero() {  // a pixel nothing reads: off the image's end, or folded as frame 0
  if constexpr (std::is_same_v<T, uint32_t>)
    return 0u;
  else
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// One frame (the realtime loop's combiner): frame 0 does not read the accumulator.
template <typename T>
__global__ __launch_bounds__(256) void accumulate(T* cur, const T* nw, size_t npix, uint32_t frame) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float* tab = fold_table<T>();
  if (i >= npix) return;
  cur[i] = fold_step(frame == 0 ? fold_zero<T>() : cur[i], nw[i], frame, tab);
}
// hrt_compute_n: the nf frames of one launch folded in frame order in one pass (frame frame0 + f is
// image f of the stack): the per-frame combiner's arithmetic, pixel by pixel, with the accumulator
// read and written once instead of once per frame.
template <typename T>
__global__ __launch_bounds__(256) void accumulate_frames(T* cur, const T* stack, size_t npix, uint32_t nf,
                                                         uint32_t frame0) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float* tab = fold_table<T>();
  if (i >= npix) return;
  T v = cur[i];
  for (uint32_t f = 0; f < nf; ++f) v = fold_step(v, stack[f * npix + i], frame0 + f, tab);
  cur[i] = v;
}

// ---- fold records (HRT_OPT_FOLD_RECORDS, hrt_compute_until) -------------------------
// The fold chain of accumulate_frames with, per frame, the record of what the fold did to the
// DISPLAYED image: pixels whose displayed word changed, the byte sum of absolute differences, the
// largest byte difference -- over the real pixels (i < real_pix; padding rows of a row-tile part are
// folded but never counted).  All integers, so the sums do not depend on the order they are taken in.
// Reduction: a wave ballots the changed lanes (no lane changed: nothing more for that frame), reduces
// sum and maximum across its lanes, lane 0 adds them to the workgroup's per-frame LDS slots; after the
// pixel walk the workgroup issues at most one global atomic triple (u32 add, u64 add, u32 max) per frame.
// The grid is sized by the CU count (launch_fold_records) and strides over the pixels, so a frame's slot
// sees at most 8 x CUs triples however large the image.  Store == false runs the chain in registers
// only (hrt_compute_until's count pass).
constexpr uint32_t kFoldMaxFrames = HRT_FOLD_RECORD_RING;  // per launch: the LDS slots
static_assert((kFoldMaxFrames & (kFoldMaxFrames - 1u)) == 0, "the ring is indexed with a mask");
template <typename T, bool Store>
__global__ __launch_bounds__(256) void fold_records(T* cur, const T* stack, size_t npix, size_t real_pix, uint32_t nf,
                                                    uint32_t frame0, hrt_fold_record* ring, uint32_t slot0,
                                                    uint32_t mask) {
  __shared__ float tab[256];
  __shared__ uint32_t s_cnt[kFoldMaxFrames], s_max[kFoldMaxFrames];
  __shared__ unsigned long long s_sum[kFoldMaxFrames];
  for (uint32_t f = threadIdx.x; f < nf; f += 256u) {
    s_cnt[f] = 0u;
    s_max[f] = 0u;
    s_sum[f] = 0ull;
  }
  unorm8_table(tab);  // (and the barrier)
  const uint32_t lane = threadIdx.x & 63u;
  const size_t stride = (size_t)gridDim.x * 256u;
  // (the walk is workgroup-uniform: every lane of a wave reaches the ballot and the shuffles)
  for (size_t base = (size_t)blockIdx.x * 256u; base < npix; base += stride) {
    const size_t i = base + threadIdx.x;
    const bool in = i < npix, real = i < real_pix;
    T v = in ? cur[i] : fold_zero<T>();
    uint32_t d = displayed_word(v);
    T nxt = in ? stack[i] : fold_zero<T>();
    for (uint32_t f = 0; f < nf; ++f) {
      const T n = nxt;
      if (f + 1u < nf && in) nxt = stack[(size_t)(f + 1u) * npix + i];
      v = fold_step(v, n, frame0 + f, tab);
      const uint32_t dw = displayed_word(v);
      const bool ch = real && dw != d;
      const unsigned long long b = __ballot(ch);
      if (b != 0ull) {
        uint32_t sad = 0u, mx = 0u;
        if (ch) {
          sad = __builtin_amdgcn_sad_u8(dw, d, 0u);
          const uint32_t b0 = __builtin_amdgcn_sad_u8(dw & 0xFFu, d & 0xFFu, 0u);
          const uint32_t b1 = __builtin_amdgcn_sad_u8(dw & 0xFF00u, d & 0xFF00u, 0u);
          const uint32_t b2 = __builtin_amdgcn_sad_u8(dw & 0xFF0000u, d & 0xFF0000u, 0u);
          const uint32_t b3 = __builtin_amdgcn_sad_u8(dw >> 24, d >> 24, 0u);
          mx = max(max(b0, b1), max(b2, b3));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          sad += (uint32_t)__shfl_xor((int)sad, off, 64);
          mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
        }
        if (lane == 0u) {
          atomicAdd(&s_cnt[f], (uint32_t)__popcll(b));
          atomicAdd(&s_sum[f], (unsigned long long)sad);
          atomicMax(&s_max[f], mx);
        }
      }
      d = dw;
    }
    if (Store && in) cur[i] = v;
  }
  __syncthreads();
  for (uint32_t f = threadIdx.x; f < nf; f += 256u) {
    if (s_cnt[f] == 0u) continue;  // (a changed pixel has a byte difference >= 1: sum and maximum are 0 too)
    hrt_fold_record* r = ring + ((slot0 + f) & mask);
    atomicAdd(&r->changed_pixels, s_cnt[f]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->abs_delta_sum), s_sum[f]);
    atomicMax(&r->max_delta, s_max[f]);
  }
}

// format conversion for hrt_read_image
__global__ __launch_bounds__(256) void rgba8_to_f32(const uint32_t* src, float4* dst, size_t npix) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix) return;
  const uint32_t v = src[i];
  dst[i] = make_float4(unorm8_to_float(v & 255u), unorm8_to_float((v >> 8) & 255u), unorm8_to_float((v >> 16) & 255u),
                       unorm8_to_float(v >> 24));
}
__global__ __launch_bounds__(256) void f32_to_rgba8(const float4* src, uint32_t* dst, size_t npix) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix) return;
  dst[i] = pack_rgba8(src[i]);
}

// ---- the present pass (RenderPassOverFrame::render, src/texture_draw_pipeline.rs:96-157) ------------
// The image as the reference's full-target quad draws it: nearest filter, flipped vertically.  One
// target row per grid.y, so the source row is wave-uniform and the stores of a row stream coalesced.
// A target pixel is the source's RGBA8 word (an RGBA32F texel packed by pack_rgba8), with bytes 0 and
// 2 swapped for a B8G8R8A8 target: one v_perm_b32 per word.
__device__ __forceinline__ uint32_t present_word(uint32_t v, uint32_t bgra) {
  return bgra ? __builtin_amdgcn_perm(v, v, 0x03000102u) : v;
}
// Where source row sy of the w-pixel-wide image starts, in rows of the buffer the kernel reads: the
// context's own image, or the root's gather buffer (hrt_present on the root of an hrt_comm_init_all
// group) -- the parts' blocks of local_rows rows in part order, read where the row-tile partition put
// each global row, so the un-interleave, the conversion and the copy of the read path are one read and
// one write.  Wave-uniform either way; 64-bit (parts x local_rows x w x 16 B may pass 2^32).
struct OwnRows {
  __device__ uint64_t operator()(uint32_t sy) const { return sy; }
};
struct GatheredRows {
  uint32_t row_tile, parts, local_rows;
  __device__ uint64_t operator()(uint32_t sy) const { return gathered_row(sy, row_tile, parts, local_rows); }
};
// Target of the image's own size: dst(x, y) = src(x, h - 1 - y) (present_sy(y, h, h)).  Four pixels per
// lane -- one 128-bit load (four float4 loads of an RGBA32F source) and one 128-bit store -- over the
// row's whole quads while the row of the target and of an RGBA8 source both start on a 16 B boundary (an
// odd width, pitch or base leaves only some rows there; with an odd width consecutive gathered rows of
// one tile alternate, and a tile's first row depends on its block); the row's last w % 4 pixels, and
// every pixel of a row that does not, go one word per lane.
template <typename T, typename Rows>
__global__ __launch_bounds__(256) void present_rows(const T* __restrict__ src, unsigned char* __restrict__ dst, uint32_t w,
                                                    uint32_t h, uint32_t pitch, uint32_t bgra, Rows row) {
  const uint32_t y = blockIdx.y;
  const T* s = src + row(h - 1u - y) * w;
  uint32_t* d = reinterpret_cast<uint32_t*>(dst + (size_t)y * pitch);
  const bool vec = (((uintptr_t)d | (sizeof(T) == 4 ? (uintptr_t)s : (uintptr_t)0)) & 15u) == 0;
  const uint32_t quads = vec ? w / 4u : 0u;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
  for (uint32_t q = t; q < quads; q += stride) {
    uint4 v;
    if constexpr (sizeof(T) == 4) {
      v = reinterpret_cast<const uint4*>(s)[q];
    } else {
      v = make_uint4(pack_rgba8(s[4u * q]), pack_rgba8(s[4u * q + 1u]), pack_rgba8(s[4u * q + 2u]),
                     pack_rgba8(s[4u * q + 3u]));
    }
    reinterpret_cast<uint4*>(d)[q] =
        make_uint4(present_word(v.x, bgra), present_word(v.y, bgra), present_word(v.z, bgra), present_word(v.w, bgra));
  }
  for (uint32_t i = quads * 4u + t; i < w; i += stride) d[i] = present_word(displayed_word(s[i]), bgra);
}
// Target of another size: sample points at the target's pixel centres, texel = floor of the centre's
// source coordinate -- the pinned integer rule (hrt_present_map.h present_sx / present_sy).
// sy of the full ws x hs image once per row (wave-uniform), sx per lane: coalesced stores, loads gathered
// along one source row.
template <typename T, typename Rows>
__global__ __launch_bounds__(256) void present_nearest(const T* __restrict__ src, uint32_t ws, uint32_t hs,
                                                       unsigned char* __restrict__ dst, uint32_t wt, uint32_t ht,
                                                       uint32_t pitch, uint32_t bgra, Rows row) {
  const uint32_t y = blockIdx.y;
  const T* s = src + row(present_sy(y, hs, ht)) * ws;
  uint32_t* d = reinterpret_cast<uint32_t*>(dst + (size_t)y * pitch);
  for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < wt; x += gridDim.x * 256u)
    d[x] = present_word(displayed_word(s[present_sx(x, ws, wt)]), bgra);
}
// hrt_accumulate_present at the image's own size: accumulate<T> whose thread also writes the folded
// pixel to the flipped target row -- the accumulator is not read again by a present pass (w * h <= 2^28).
template <typename T>
__global__ __launch_bounds__(256) void accumulate_present(T* cur, const T* nw, uint32_t w, uint32_t h, uint32_t frame,
                                                          unsigned char* __restrict__ dst, uint32_t pitch,
                                                          uint32_t bgra) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const float* tab = fold_table<T>();
  if (i >= w * h) return;
  const T v = fold_step(frame == 0 ? fold_zero<T>() : cur[i], nw[i], frame, tab);
  cur[i] = v;
  const uint32_t y = i / w, x = i - y * w;
  reinterpret_cast<uint32_t*>(dst + (size_t)(h - 1u - y) * pitch)[x] = present_word(displayed_word(v), bgra);
}

// Row-tile framebuffer assembly after the gather: global row y lives in part
// (y / row_tile) % parts at local row (y / row_tile / parts) * row_tile + y % row_tile.  One 4-byte word
// per lane; grid.y = rows, so the row arithmetic is wave-uniform and both sides stream coalesced.
__global__ __launch_bounds__(256) void assemble_rows(const uint32_t* __restrict__ gathered, uint32_t* __restrict__ frame,
                                                     uint32_t row_words, uint32_t local_rows, uint32_t row_tile,
                                                     uint32_t parts) {
  const uint32_t y = blockIdx.y;
  const uint32_t t = y / row_tile;
  const uint32_t part = t % parts;
  const uint32_t lr = (t / parts) * row_tile + y % row_tile;
  const uint32_t* src = gathered + ((size_t)part * local_rows + lr) * row_words;
  uint32_t* dst = frame + (size_t)y * row_words;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < row_words; i += gridDim.x * 256) dst[i] = src[i];
}

// ---- launch wrappers (host) ----------------------------------------------------------------------
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

// The one place a format becomes a pixel type: f(px) with px a value of the image's pixel type.
template <typename F>
static void with_pixel_type(bool f32, F f) {
  if (f32)
    f(float4{});
  else
    f(uint32_t{});
}

hipError_t launch_clear(void* img, bool f32, size_t npix, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  with_pixel_type(f32, [&](auto px) {
    using T = decltype(px);
    clear_kernel<T><<<blocks_for(npix), 256, 0, stream>>>(static_cast<T*>(img), npix);
  });
  return hipGetLastError();
}

hipError_t launch_accumulate(void* cur, const void* nw, bool f32, size_t npix, uint32_t frame, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  with_pixel_type(f32, [&](auto px) {
    using T = decltype(px);
    accumulate<T><<<blocks_for(npix), 256, 0, stream>>>(static_cast<T*>(cur), static_cast<const T*>(nw), npix, frame);
  });
  return hipGetLastError();
}

hipError_t launch_accumulate_frames(void* cur, const void* stack, bool f32, size_t npix, uint32_t nf, uint32_t frame0,
                                    hipStream_t stream) {
  if (npix == 0 || nf == 0) return hipSuccess;
  with_pixel_type(f32, [&](auto px) {
    using T = decltype(px);
    accumulate_frames<T>
        <<<blocks_for(npix), 256, 0, stream>>>(static_cast<T*>(cur), static_cast<const T*>(stack), npix, nf, frame0);
  });
  return hipGetLastError();
}

hipError_t launch_fold_records(void* cur, const void* stack, bool f32, size_t npix, size_t real_pix, uint32_t nf,
                               uint32_t frame0, bool store, hrt_fold_record* ring, uint32_t slot0, uint32_t num_cus,
                               hipStream_t stream) {
  if (nf == 0) return hipSuccess;
  if (nf > kFoldMaxFrames || !ring || real_pix > npix || npix == 0) return hipErrorInvalidValue;
  // eight workgroups of four waves per CU (full occupancy beside 17 KiB of LDS each), never more than the pixels need
  const unsigned int grid = std::min<unsigned int>(blocks_for(npix), std::max(1u, num_cus) * 8u);
  const uint32_t mask = kFoldMaxFrames - 1u;
  slot0 &= mask;
  with_pixel_type(f32, [&](auto px) {
    using T = decltype(px);
    T* c = static_cast<T*>(cur);
    const T* s = static_cast<const T*>(stack);
    if (store)
      fold_records<T, true><<<grid, 256, 0, stream>>>(c, s, npix, real_pix, nf, frame0, ring, slot0, mask);
    else
      fold_records<T, false><<<grid, 256, 0, stream>>>(c, s, npix, real_pix, nf, frame0, ring, slot0, mask);
  });
  return hipGetLastError();
}

hipError_t launch_convert(const void* src, bool src_f32, void* dst, size_t npix, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  if (src_f32)
    f32_to_rgba8<<<blocks_for(npix), 256, 0, stream>>>(static_cast<const float4*>(src), static_cast<uint32_t*>(dst), npix);
  else
    rgba8_to_f32<<<blocks_for(npix), 256, 0, stream>>>(static_cast<const uint32_t*>(src), static_cast<float4*>(dst), npix);
  return hipGetLastError();
}

// present_rows at the image's own size (a lane moves four pixels; rows off the 16 B grid loop), else present_nearest
template <typename Rows>
static void present_launch(const void* src, bool f32, uint32_t ws, uint32_t hs, Rows row, const PresentTarget& t,
                           hipStream_t stream) {
  with_pixel_type(f32, [&](auto px) {
    using T = decltype(px);
    if (t.width == ws && t.height == hs) {
      const dim3 g(((t.width + 3) / 4 + 255) / 256, t.height, 1);
      present_rows<T, Rows><<<g, 256, 0, stream>>>(static_cast<const T*>(src), t.dst, ws, hs, t.pitch, t.bgra, row);
    } else {
      const dim3 g((t.width + 255) / 256, t.height, 1);
      present_nearest<T, Rows>
          <<<g, 256, 0, stream>>>(static_cast<const T*>(src), ws, hs, t.dst, t.width, t.height, t.pitch, t.bgra, row);
    }
  });
}

hipError_t launch_present(const void* src, bool f32, uint32_t ws, uint32_t hs, const PresentTarget& t,
                          hipStream_t stream) {
  // (grid.y = target rows; the checks of hrt_present, repeated where the launch is shaped)
  if (ws == 0 || hs == 0 || t.width == 0 || t.height == 0 || t.height > 65535u || t.pitch / 4 < t.width || !t.dst)
    return hipErrorInvalidValue;
  present_launch(src, f32, ws, hs, OwnRows{}, t, stream);
  return hipGetLastError();
}

hipError_t launch_present_gathered(const GatheredImage& g, const PresentTarget& t, hipStream_t stream) {
  if (g.width == 0 || g.height == 0 || t.width == 0 || t.height == 0 || t.height > 65535u || t.pitch / 4 < t.width ||
      !t.dst || !g.src)
    return hipErrorInvalidValue;
  // (launch_assemble_rows' bound: every global row below height lies inside its part's local rows)
  if (g.parts == 0 || g.row_tile == 0 ||
      (uint64_t)((g.height - 1) / g.row_tile / g.parts + 1) * g.row_tile > g.local_rows)
    return hipErrorInvalidValue;
  present_launch(g.src, g.f32, g.width, g.height, GatheredRows{g.row_tile, g.parts, g.local_rows}, t, stream);
  return hipGetLastError();
}

hipError_t launch_accumulate_present(void* cur, const void* nw, bool f32, uint32_t w, uint32_t h, uint32_t frame,
                                     const PresentTarget& t, hipStream_t stream) {
  if (w == 0 || h == 0 || t.width != w || t.height != h || (uint64_t)w * h > (1ull << 28) || t.pitch / 4 < w || !t.dst)
    return hipErrorInvalidValue;
  with_pixel_type(f32, [&](auto px) {
    using T = decltype(px);
    accumulate_present<T><<<blocks_for((size_t)w * h), 256, 0, stream>>>(static_cast<T*>(cur), static_cast<const T*>(nw),
                                                                        w, h, frame, t.dst, t.pitch, t.bgra);
  });
  return hipGetLastError();
}

hipError_t launch_assemble_rows(const uint32_t* gathered, uint32_t* frame, uint32_t row_words, uint32_t height,
                                uint32_t local_rows, uint32_t row_tile, uint32_t parts, hipStream_t stream) {
  if (row_words == 0 || height == 0) return hipSuccess;
  if (parts == 0 || row_tile == 0 || (uint64_t)((height - 1) / row_tile / parts + 1) * row_tile > local_rows)
    return hipErrorInvalidValue;  // some global row would read outside its part's local rows
  const dim3 g(std::min<uint32_t>((row_words + 255) / 256, 64), height, 1);
  assemble_rows<<<g, 256, 0, stream>>>(gathered, frame, row_words, local_rows, row_tile, parts);
  return hipGetLastError();
}

}  // namespace hrt
