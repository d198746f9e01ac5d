// motion_map_test: the HIP-free coordinate arithmetic of the reprojection under object motion
// (epq_raytracer_amd/csrc/hrt_motion_map.h) as a stand-alone program; tests/test_motion_ref.py compares its output
// word for word with the numpy restatement (tests/motion_ref.py).  Built plain and under ASan + UBSan.
//
// usage: motion_map_test < records > words
// Input: records of 30 float32 words: prev_pose[12], cur_pose[12], a point[3], a normal[3].  Output per record, 19
// uint32 words: G[12] = motion_between(prev_pose, cur_pose), whether the poses differ, motion_point(G, point)[3],
// motion_normal(G, normal)[3].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hrt_motion_map.h"

int main() {
  std::vector<float> in(30);
  std::vector<uint32_t> out(19);
  while (std::fread(in.data(), 4, in.size(), stdin) == in.size()) {
    float g[12], p[3], n[3];
    const bool differ = hrt::motion_between(in.data(), in.data() + 12, g);
    hrt::motion_point(g, in.data() + 24, p);
    hrt::motion_normal(g, in.data() + 27, n);
    std::memcpy(out.data(), g, sizeof g);
    out[12] = differ ? 1u : 0u;
    std::memcpy(out.data() + 13, p, sizeof p);
    std::memcpy(out.data() + 16, n, sizeof n);
    if (std::fwrite(out.data(), 4, out.size(), stdout) != out.size()) return 1;
  }
  return 0;
}
