// hrt_motion_map.h -- the coordinate arithmetic of the reprojection under object motion (hrt_reproject_motion;
// DESIGN.md §2 S21, §36) and of hrt_host_motion_between, shared by the kernel (hrt_history.hip), the host helper
// (hrt_host.cpp) and a plain C++ test program (tests/cpp/motion_map_test.cpp): no HIP header is needed to compile it.
//
// G is hrt_motion.m: a column-major 3x4 [L | b], previous world point = L * current world point + b.  Every
// function is S21's arithmetic: one rounded binary32 operation per written operation, in the written order.  Every
// user is built with -ffp-contract=off.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HRT_MOMAP_FN __host__ __device__ inline
#else
#define HRT_MOMAP_FN inline
#endif

namespace hrt {

// S21 step 4: P'.k = ((G[k] * P.x + G[3 + k] * P.y) + G[6 + k] * P.z) + G[9 + k].
HRT_MOMAP_FN void motion_point(const float g[12], const float p[3], float out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = ((g[k] * p[0] + g[3 + k] * p[1]) + g[6 + k] * p[2]) + g[9 + k];
}

// S21 step 8: n'.k = (G[k] * n.x + G[3 + k] * n.y) + G[6 + k] * n.z (not renormalised).
HRT_MOMAP_FN void motion_normal(const float g[12], const float n[3], float out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = (g[k] * n[0] + g[3 + k] * n[1]) + g[6 + k] * n[2];
}

// hrt_host_motion_between's G = prev o cur^-1 of two column-major 3x4 poses [R | t] whose linear parts are rotations:
// L[r][c] = (Rp[r][0] * Rc[c][0] + Rp[r][1] * Rc[c][1]) + Rp[r][2] * Rc[c][2], b = tp - L * tc with
// (L * tc).r = (L[r][0] * tc.x + L[r][1] * tc.y) + L[r][2] * tc.z.  Returns whether the poses differ in any byte.
HRT_MOMAP_FN bool motion_between(const float prev_pose[12], const float cur_pose[12], float g[12]) {
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r)
      g[3 * c + r] = (prev_pose[r] * cur_pose[c] + prev_pose[3 + r] * cur_pose[3 + c]) + prev_pose[6 + r] * cur_pose[6 + c];
  for (int r = 0; r < 3; ++r) {
    const float lt = (g[r] * cur_pose[9] + g[3 + r] * cur_pose[10]) + g[6 + r] * cur_pose[11];
    g[9 + r] = prev_pose[9 + r] - lt;
  }
  bool differ = false;
  for (int i = 0; i < 12; ++i) {
    uint32_t a, b;
    memcpy(&a, prev_pose + i, 4);
    memcpy(&b, cur_pose + i, 4);
    differ = differ || a != b;
  }
  return differ;
}

}  // namespace hrt
