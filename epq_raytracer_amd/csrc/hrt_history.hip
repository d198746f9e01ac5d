// hrt_history.hip -- gfx950 kernels of the temporal history (hrt_history.h):
// fold_history, the combiner with a per-pixel frame number, and reproject, which carries the accumulator and
// the count image across a change of view; and their forms that carry the luminance moments image M of the
// variance-guided denoise beside them (hrt_variance.h): fold_history_moments and
// reproject<.., true>.
//
// S15 is pinned operation by operation and the unit is built with -ffp-contract=off: every statement of the
// reprojection below is one rounded float operation of the spec, in its order (hdot / hcross are S15's own
// spellings without fma, not hrt_math.h's S2 forms); '/' and sqrt are the correctly rounded ones (S4).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hip_raytrace.h"
#include "hrt_history.h"
#include "hrt_history_fold.h"
#include "hrt_motion_map.h"
#include "hrt_variance.h"
#include "hrt_math.h"

namespace hrt {

// (the fold's per-pixel device functions -- hist_step, hist_next, moments_step, hist_key -- live in
// hrt_history_fold.h, shared with hrt_refine.hip)


// One pixel per lane in RGBA32F mode (a texel is one 128-bit access).  In RGBA8 mode a lane takes the `quads`
// whole groups of four pixels with one 128-bit access per array (quads = npix / 4 when all three arrays start
// on a 16-byte boundary, else 0) and the remaining pixels go one word per lane.
template <typename T>
__global__ __launch_bounds__(256) void fold_history(T* cur, const T* nw, uint32_t* cnt, size_t npix, size_t quads,
                                                    uint32_t max_history) {
  const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
  if constexpr (std::is_same_v<T, uint32_t>) {
    __shared__ float tab[256];
    tab[threadIdx.x] = unorm8_to_float(threadIdx.x);
    __syncthreads();
    if (t < quads) {
      const uint4 n = reinterpret_cast<const uint4*>(cnt)[t];
      const uint4 v = reinterpret_cast<const uint4*>(nw)[t];
      uint4 c = make_uint4(0u, 0u, 0u, 0u);
      if ((n.x | n.y | n.z | n.w) != 0u) c = reinterpret_cast<const uint4*>(cur)[t];
      reinterpret_cast<uint4*>(cur)[t] = make_uint4(hist_step(c.x, v.x, n.x, tab), hist_step(c.y, v.y, n.y, tab),
                                                    hist_step(c.z, v.z, n.z, tab), hist_step(c.w, v.w, n.w, tab));
      reinterpret_cast<uint4*>(cnt)[t] = make_uint4(hist_next(n.x, max_history), hist_next(n.y, max_history),
                                                    hist_next(n.z, max_history), hist_next(n.w, max_history));
    }
    const size_t i = quads * 4u + t;
    if (i < npix) {
      const uint32_t n = cnt[i];
      cur[i] = hist_step(n == 0u ? 0u : cur[i], nw[i], n, tab);
      cnt[i] = hist_next(n, max_history);
    }
  } else {
    if (t >= npix) return;
    const uint32_t n = cnt[t];
    cur[t] = hist_step(n == 0u ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : cur[t], nw[t], n, nullptr);
    cnt[t] = hist_next(n, max_history);
  }
}


// fold_history with the moments image: the same lanes and the same 128-bit accesses of cur, nw and cnt; a lane of
// the RGBA8 quads takes its four pixels' moments as two 128-bit accesses of two pixels each, a float lane (and an
// RGBA8 remainder lane) its pixel's pair as one 64-bit access.
template <typename T>
__global__ __launch_bounds__(256) void fold_history_moments(T* cur, const T* nw, uint32_t* cnt, float2* mom, size_t npix,
                                                            size_t quads, uint32_t max_history) {
  const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
  if constexpr (std::is_same_v<T, uint32_t>) {
    __shared__ float tab[256];
    tab[threadIdx.x] = unorm8_to_float(threadIdx.x);
    __syncthreads();
    if (t < quads) {
      const uint4 n = reinterpret_cast<const uint4*>(cnt)[t];
      const uint4 v = reinterpret_cast<const uint4*>(nw)[t];
      uint4 c = make_uint4(0u, 0u, 0u, 0u);
      float4 ma = make_float4(0.0f, 0.0f, 0.0f, 0.0f), mb = ma;
      if ((n.x | n.y | n.z | n.w) != 0u) {
        c = reinterpret_cast<const uint4*>(cur)[t];
        ma = reinterpret_cast<const float4*>(mom)[2 * t];
        mb = reinterpret_cast<const float4*>(mom)[2 * t + 1];
      }
      reinterpret_cast<uint4*>(cur)[t] = make_uint4(hist_step(c.x, v.x, n.x, tab), hist_step(c.y, v.y, n.y, tab),
                                                    hist_step(c.z, v.z, n.z, tab), hist_step(c.w, v.w, n.w, tab));
      reinterpret_cast<uint4*>(cnt)[t] = make_uint4(hist_next(n.x, max_history), hist_next(n.y, max_history),
                                                    hist_next(n.z, max_history), hist_next(n.w, max_history));
      const float2 m0 = moments_step(make_float2(ma.x, ma.y), v.x, n.x, tab);
      const float2 m1 = moments_step(make_float2(ma.z, ma.w), v.y, n.y, tab);
      const float2 m2 = moments_step(make_float2(mb.x, mb.y), v.z, n.z, tab);
      const float2 m3 = moments_step(make_float2(mb.z, mb.w), v.w, n.w, tab);
      reinterpret_cast<float4*>(mom)[2 * t] = make_float4(m0.x, m0.y, m1.x, m1.y);
      reinterpret_cast<float4*>(mom)[2 * t + 1] = make_float4(m2.x, m2.y, m3.x, m3.y);
    }
    const size_t i = quads * 4u + t;
    if (i < npix) {
      const uint32_t n = cnt[i];
      const uint32_t v = nw[i];
      cur[i] = hist_step(n == 0u ? 0u : cur[i], v, n, tab);
      cnt[i] = hist_next(n, max_history);
      mom[i] = moments_step(n == 0u ? make_float2(0.0f, 0.0f) : mom[i], v, n, tab);
    }
  } else {
    if (t >= npix) return;
    const uint32_t n = cnt[t];
    const float4 v = nw[t];
    cur[t] = hist_step(n == 0u ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : cur[t], v, n, nullptr);
    cnt[t] = hist_next(n, max_history);
    mom[t] = moments_step(n == 0u ? make_float2(0.0f, 0.0f) : mom[t], v, n, nullptr);
  }
}

__global__ __launch_bounds__(256) void fill_moments(float2* mom, size_t npix, float m1, float m2) {
  const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (t < npix) mom[t] = make_float2(m1, m2);
}

// ---- the reprojection ------------------------------------------------------------------------------------
constexpr uint32_t kTileW = 32, kTileH = 8;  // one pixel per thread of a 256-thread workgroup, a wave = 2 rows

// S15's dot and cross: products and sums in the written order, no fma.
__device__ __forceinline__ float hdot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ f3 hcross(f3 a, f3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// The rgb of a texel as S14's C0 defines it.
__device__ __forceinline__ f3 texel_rgb(uint32_t v) {
  return {unorm8_to_float(v & 255u), unorm8_to_float((v >> 8) & 255u), unorm8_to_float((v >> 16) & 255u)};
}
__device__ __forceinline__ f3 texel_rgb(float4 v) { return {v.x, v.y, v.z}; }
template <typename T>
__device__ __forceinline__ T texel_cleared() {
  if constexpr (std::is_same_v<T, uint32_t>)
    return 255u << 24;
  else
    return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
}

// What the kernel takes of an hrt_view, by value.
struct ViewK {
  f3 o;        // cam_pos
  float m[9];  // mat3 of cam_alignment_mat, column-major: m[3 c + r]
  f3 first, dx, dy;
};

// What tap acceptance needs of the current pixel (S15 step 8).
struct ReprojCentre {
  uint32_t kc;
  float te, tol_te;
  f3 nc;
  float min_dot;
};
// Step 8 for source pixel j, which lies inside the image.
__device__ __forceinline__ bool tap_accepted(const ReprojCentre& c, const uint32_t* __restrict__ cnt,
                                             const float4* __restrict__ prev_hits, size_t j, uint32_t& nj) {
  nj = cnt[j];
  if (nj == 0u) return false;
  const float4 a = prev_hits[2 * j];
  if (hist_key(a) != c.kc) return false;
  if (c.kc != 0u) {
    const float4 b = prev_hits[2 * j + 1];
    if (!(fabsf(c.te - a.x) <= c.tol_te)) return false;
    if (!(hdot(c.nc, mk(b.x, b.y, b.z)) >= c.min_dot)) return false;
  }
  return true;
}

// One thread per pixel, row-major 32-wide workgroup rows: after a small camera move the sources of a wave's
// two rows are neighbours again, so their texels, counts and hit records share cache lines.
// Moments (S16): the moments image is carried beside them -- mom_out[i] <- the same taps of mom_in with the same
// weights, in the same order, over the same wsum; (0, 0) for a rejected pixel.  Without it the two pointers are
// not touched.
//
// Motion (S21): the pixel's object may carry a rigid motion G between the two frames -- a kind-1 hit's entry is
// spheres[hit.index], a kind-2 hit's meshes[hit.mesh], 64-byte hrt_motion records read as four 128-bit words.  An
// index at or past its count, an entry whose flags are 0 and a miss are static and take S15's statements; a moving
// pixel puts its point through G before step 4's subtraction and its normal through G's linear part before step 8.
// Neighbouring pixels mostly share an object, so a wave's loads of the entry mostly hit one or two cache lines.
// The plain forms (Motion false) take an empty last argument: their code is what it was before the motion forms
// existed (profiles/motion_resources.txt).
struct MotionTabK {
  const float4* spheres;
  const float4* meshes;
  uint32_t n_spheres, n_meshes;
};
struct NoMotionK {};
template <bool Motion>
using MotionArgK = std::conditional_t<Motion, MotionTabK, NoMotionK>;

template <typename T, uint32_t Filter, bool Moments, bool Motion>
__global__ __launch_bounds__(256) void reproject(const T* __restrict__ acc_in, const uint32_t* __restrict__ cnt_in,
                                                 T* __restrict__ acc_out, uint32_t* __restrict__ cnt_out,
                                                 const float4* __restrict__ prev_hits,
                                                 const float4* __restrict__ cur_hits, ViewK vp, ViewK vc, uint32_t w,
                                                 uint32_t h, float tol, float min_dot,
                                                 const float2* __restrict__ mom_in, float2* __restrict__ mom_out,
                                                 MotionArgK<Motion> tab) {
  const uint32_t x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1u));
  const uint32_t y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  if (x >= w || y >= h) return;
  const size_t i = (size_t)y * w + x;
  const float4 ha = cur_hits[2 * i], hb = cur_hits[2 * i + 1];
  ReprojCentre c;
  c.kc = hist_key(ha);
  c.nc = mk(hb.x, hb.y, hb.z);
  c.min_dot = min_dot;
  // steps 1-3: the un-jittered direction of the pixel's centre in the current view
  const float fx = (float)x, fy = (float)y;
  const f3 cc = {(vc.first.x + vc.dx.x * fx) + vc.dy.x * fy, (vc.first.y + vc.dx.y * fx) + vc.dy.y * fy,
                 (vc.first.z + vc.dx.z * fx) + vc.dy.z * fy};
  const f3 d = {(vc.m[0] * cc.x + vc.m[3] * cc.y) + vc.m[6] * cc.z, (vc.m[1] * cc.x + vc.m[4] * cc.y) + vc.m[7] * cc.z,
                (vc.m[2] * cc.x + vc.m[5] * cc.y) + vc.m[8] * cc.z};
  const float len = __builtin_sqrtf(hdot(d, d));
  const f3 dn = {d.x / len, d.y / len, d.z / len};
  // step 4: the surface point relative to the previous camera, or the direction alone for a miss
  f3 v = dn;
  c.te = 0.0f;
  c.tol_te = 0.0f;
  if (c.kc != 0u) {
    f3 p = {vc.o.x + dn.x * ha.x, vc.o.y + dn.y * ha.x, vc.o.z + dn.z * ha.x};
    if constexpr (Motion) {
      const uint32_t kind = __float_as_uint(ha.y);
      const uint32_t idx = kind == 1u ? __float_as_uint(ha.z) : __float_as_uint(ha.w);
      const float4* e = kind == 1u ? tab.spheres : tab.meshes;
      const uint32_t cnt = kind == 1u ? tab.n_spheres : tab.n_meshes;
      if (idx < cnt) {
        e += (size_t)idx * 4u;
        if (__float_as_uint(e[3].x) != 0u) {
          const float4 g0 = e[0], g1 = e[1], g2 = e[2];
          const float g[12] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x, g2.y, g2.z, g2.w};
          const float pin[3] = {p.x, p.y, p.z}, nin[3] = {c.nc.x, c.nc.y, c.nc.z};
          float pout[3], nout[3];
          motion_point(g, pin, pout);
          motion_normal(g, nin, nout);
          p = {pout[0], pout[1], pout[2]};
          c.nc = {nout[0], nout[1], nout[2]};
        }
      }
    }
    v = {p.x - vp.o.x, p.y - vp.o.y, p.z - vp.o.z};
    c.te = __builtin_sqrtf(hdot(v, v));
    c.tol_te = tol * c.te;
  }
  // steps 5-7: into the previous camera's space and onto its grid
  const f3 q = {hdot(mk(vp.m[0], vp.m[1], vp.m[2]), v), hdot(mk(vp.m[3], vp.m[4], vp.m[5]), v),
                hdot(mk(vp.m[6], vp.m[7], vp.m[8]), v)};
  const f3 n = hcross(vp.dx, vp.dy);
  const float s = hdot(vp.first, n) / hdot(q, n);
  T texel = texel_cleared<T>();
  uint32_t count = 0u;
  float2 mom = make_float2(0.0f, 0.0f);
  if (s > 0.0f) {
    const f3 r = {q.x * s - vp.first.x, q.y * s - vp.first.y, q.z * s - vp.first.z};
    const float u = hdot(r, vp.dx) / hdot(vp.dx, vp.dx);
    const float wv = hdot(r, vp.dy) / hdot(vp.dy, vp.dy);
    const float xmax = (float)(w - 1u), ymax = (float)(h - 1u);
    if constexpr (Filter == HRT_REPROJECT_NEAREST) {
      const float ix = __builtin_floorf(u + 0.5f), iy = __builtin_floorf(wv + 0.5f);
      if (ix >= 0.0f && ix <= xmax && iy >= 0.0f && iy <= ymax) {
        const size_t j = (size_t)(uint32_t)iy * w + (uint32_t)ix;
        uint32_t nj;
        if (tap_accepted(c, cnt_in, prev_hits, j, nj)) {
          texel = acc_in[j];
          count = nj;
          if constexpr (Moments) mom = mom_in[j];
        }
      }
    } else {
      const float x0 = __builtin_floorf(u), y0 = __builtin_floorf(wv);
      if (x0 >= -1.0f && x0 <= xmax && y0 >= -1.0f && y0 <= ymax) {
        const float a = u - x0, b = wv - y0;
        const int64_t ix0 = (int64_t)x0, iy0 = (int64_t)y0;
        float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
        float am1 = 0.0f, am2 = 0.0f;
        uint32_t nmin = 0xFFFFFFFFu;
        bool used = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ex = e & 1, ey = e >> 1;
          const float wx = ex ? a : 1.0f - a, wy = ey ? b : 1.0f - b;
          const float wt = wx * wy;
          const int64_t jx = ix0 + ex, jy = iy0 + ey;
          if (!(wt > 0.0f) || jx < 0 || jx >= (int64_t)w || jy < 0 || jy >= (int64_t)h) continue;
          const size_t j = (size_t)jy * w + (size_t)jx;
          uint32_t nj;
          if (!tap_accepted(c, cnt_in, prev_hits, j, nj)) continue;
          const f3 cj = texel_rgb(acc_in[j]);
          ar = ar + wt * cj.x;
          ag = ag + wt * cj.y;
          ab = ab + wt * cj.z;
          if constexpr (Moments) {
            const float2 mj = mom_in[j];
            am1 = am1 + wt * mj.x;
            am2 = am2 + wt * mj.y;
          }
          wsum = wsum + wt;
          nmin = nj < nmin ? nj : nmin;
          used = true;
        }
        if (used) {
          const float r8 = ar / wsum, g8 = ag / wsum, b8 = ab / wsum;
          if constexpr (std::is_same_v<T, uint32_t>)
            texel = unorm8(r8) | (unorm8(g8) << 8) | (unorm8(b8) << 16) | (255u << 24);
          else
            texel = make_float4(r8, g8, b8, 1.0f);
          count = nmin;
          if constexpr (Moments) mom = make_float2(am1 / wsum, am2 / wsum);
        }
      }
    }
  }
  acc_out[i] = texel;
  cnt_out[i] = count;
  if constexpr (Moments) mom_out[i] = mom;
}

// ---- launch wrappers (host) ------------------------------------------------------------------------------
hipError_t launch_fold_history(void* cur, const void* nw, uint32_t* cnt, bool f32, size_t npix, uint32_t max_history,
                               hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  if (!cur || !nw || !cnt || max_history == 0 || max_history > kHistoryMax) return hipErrorInvalidValue;
  if (f32) {
    if ((((uintptr_t)cur | (uintptr_t)nw) & 15u) != 0) return hipErrorInvalidValue;
    fold_history<float4><<<(unsigned)((npix + 255) / 256), 256, 0, stream>>>(
        static_cast<float4*>(cur), static_cast<const float4*>(nw), cnt, npix, 0, max_history);
  } else {
    const bool vec = (((uintptr_t)cur | (uintptr_t)nw | (uintptr_t)cnt) & 15u) == 0;
    const size_t quads = vec ? npix / 4 : 0, rest = npix - 4 * quads;
    const size_t threads = quads > rest ? quads : rest;
    fold_history<uint32_t><<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(
        static_cast<uint32_t*>(cur), static_cast<const uint32_t*>(nw), cnt, npix, quads, max_history);
  }
  return hipGetLastError();
}

static ViewK view_k(const hrt_view& v) {
  ViewK k;
  k.o = {v.cam_pos[0], v.cam_pos[1], v.cam_pos[2]};
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) k.m[3 * c + r] = v.cam_alignment_mat[4 * c + r];
  k.first = {v.grid_first[0], v.grid_first[1], v.grid_first[2]};
  k.dx = {v.grid_dx[0], v.grid_dx[1], v.grid_dx[2]};
  k.dy = {v.grid_dy[0], v.grid_dy[1], v.grid_dy[2]};
  return k;
}

template <typename T, bool Moments>
static void reproject_launch(const ReprojectPass& p, const float* mom_in, float* mom_out, dim3 grid, hipStream_t stream,
                             const MotionTables* motion) {
  const T* ain = static_cast<const T*>(p.acc_in);
  T* aout = static_cast<T*>(p.acc_out);
  const float4* ph = reinterpret_cast<const float4*>(p.prev_hits);
  const float4* ch = reinterpret_cast<const float4*>(p.cur_hits);
  const ViewK vp = view_k(p.prev), vc = view_k(p.cur);
  const float2* mi = reinterpret_cast<const float2*>(mom_in);
  float2* mo = reinterpret_cast<float2*>(mom_out);
  if (motion) {
    const MotionTabK tab{reinterpret_cast<const float4*>(motion->spheres), reinterpret_cast<const float4*>(motion->meshes),
                         motion->n_spheres, motion->n_meshes};
    if (p.filter == HRT_REPROJECT_NEAREST)
      reproject<T, HRT_REPROJECT_NEAREST, Moments, true><<<grid, 256, 0, stream>>>(
          ain, p.cnt_in, aout, p.cnt_out, ph, ch, vp, vc, p.w, p.h, p.depth_tolerance, p.min_normal_dot, mi, mo, tab);
    else
      reproject<T, HRT_REPROJECT_BILINEAR, Moments, true><<<grid, 256, 0, stream>>>(
          ain, p.cnt_in, aout, p.cnt_out, ph, ch, vp, vc, p.w, p.h, p.depth_tolerance, p.min_normal_dot, mi, mo, tab);
    return;
  }
  if (p.filter == HRT_REPROJECT_NEAREST)
    reproject<T, HRT_REPROJECT_NEAREST, Moments, false><<<grid, 256, 0, stream>>>(
        ain, p.cnt_in, aout, p.cnt_out, ph, ch, vp, vc, p.w, p.h, p.depth_tolerance, p.min_normal_dot, mi, mo, NoMotionK{});
  else
    reproject<T, HRT_REPROJECT_BILINEAR, Moments, false><<<grid, 256, 0, stream>>>(
        ain, p.cnt_in, aout, p.cnt_out, ph, ch, vp, vc, p.w, p.h, p.depth_tolerance, p.min_normal_dot, mi, mo, NoMotionK{});
}

static hipError_t reproject_dispatch(const ReprojectPass& p, const float* mom_in, float* mom_out, hipStream_t stream,
                                     const MotionTables* motion = nullptr) {
  if (motion && (p.w != 0 && p.h != 0)) {
    if ((motion->n_spheres && !motion->spheres) || (motion->n_meshes && !motion->meshes)) return hipErrorInvalidValue;
    if ((((uintptr_t)motion->spheres | (uintptr_t)motion->meshes) & 15u) != 0) return hipErrorInvalidValue;
  }
  if (p.w == 0 || p.h == 0) return hipSuccess;
  if (!p.acc_in || !p.cnt_in || !p.acc_out || !p.cnt_out || !p.prev_hits || !p.cur_hits) return hipErrorInvalidValue;
  if (p.acc_in == p.acc_out || p.cnt_in == p.cnt_out) return hipErrorInvalidValue;
  if (p.filter != HRT_REPROJECT_NEAREST && p.filter != HRT_REPROJECT_BILINEAR) return hipErrorInvalidValue;
  if ((((uintptr_t)p.prev_hits | (uintptr_t)p.cur_hits) & 15u) != 0) return hipErrorInvalidValue;
  const dim3 grid((p.w + kTileW - 1) / kTileW, (p.h + kTileH - 1) / kTileH, 1);
  // (grid.y = tile rows; float(w - 1) and float(h - 1), the bounds of S15's steps 9 and 10, must be exact)
  if (grid.y > 65535u || p.w > (1u << 24)) return hipErrorInvalidValue;
  if (mom_in) {
    if (p.f32)
      reproject_launch<float4, true>(p, mom_in, mom_out, grid, stream, motion);
    else
      reproject_launch<uint32_t, true>(p, mom_in, mom_out, grid, stream, motion);
  } else if (p.f32) {
    reproject_launch<float4, false>(p, nullptr, nullptr, grid, stream, motion);
  } else {
    reproject_launch<uint32_t, false>(p, nullptr, nullptr, grid, stream, motion);
  }
  return hipGetLastError();
}

hipError_t launch_reproject(const ReprojectPass& p, hipStream_t stream) {
  return reproject_dispatch(p, nullptr, nullptr, stream);
}

hipError_t launch_reproject_moments(const ReprojectPass& p, const float* mom_in, float* mom_out, hipStream_t stream) {
  if (p.w == 0 || p.h == 0) return hipSuccess;
  if (!mom_in || !mom_out || mom_in == mom_out || (((uintptr_t)mom_in | (uintptr_t)mom_out) & 7u) != 0)
    return hipErrorInvalidValue;
  return reproject_dispatch(p, mom_in, mom_out, stream);
}

hipError_t launch_reproject_motion(const ReprojectPass& p, const MotionTables& motion, const float* mom_in, float* mom_out,
                                   hipStream_t stream) {
  if (p.w == 0 || p.h == 0) return hipSuccess;
  if ((mom_in == nullptr) != (mom_out == nullptr)) return hipErrorInvalidValue;
  if (mom_in && (mom_in == mom_out || (((uintptr_t)mom_in | (uintptr_t)mom_out) & 7u) != 0)) return hipErrorInvalidValue;
  return reproject_dispatch(p, mom_in, mom_out, stream, &motion);
}

hipError_t launch_fold_history_moments(void* cur, const void* nw, uint32_t* cnt, float* mom, bool f32, size_t npix,
                                       uint32_t max_history, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  if (!cur || !nw || !cnt || !mom || max_history == 0 || max_history > kHistoryMax) return hipErrorInvalidValue;
  if (((uintptr_t)mom & 15u) != 0) return hipErrorInvalidValue;
  float2* m = reinterpret_cast<float2*>(mom);
  if (f32) {
    if ((((uintptr_t)cur | (uintptr_t)nw) & 15u) != 0) return hipErrorInvalidValue;
    fold_history_moments<float4><<<(unsigned)((npix + 255) / 256), 256, 0, stream>>>(
        static_cast<float4*>(cur), static_cast<const float4*>(nw), cnt, m, npix, 0, max_history);
  } else {
    const bool vec = (((uintptr_t)cur | (uintptr_t)nw | (uintptr_t)cnt) & 15u) == 0;
    const size_t quads = vec ? npix / 4 : 0, rest = npix - 4 * quads;
    const size_t threads = quads > rest ? quads : rest;
    fold_history_moments<uint32_t><<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(
        static_cast<uint32_t*>(cur), static_cast<const uint32_t*>(nw), cnt, m, npix, quads, max_history);
  }
  return hipGetLastError();
}

hipError_t launch_fill_moments(float* mom, size_t npix, float m1, float m2, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  if (!mom || ((uintptr_t)mom & 7u) != 0) return hipErrorInvalidValue;
  fill_moments<<<(unsigned)((npix + 255) / 256), 256, 0, stream>>>(reinterpret_cast<float2*>(mom), npix, m1, m2);
  return hipGetLastError();
}

}  // namespace hrt
