// launch_plan_test.cpp -- prints the launch plans of epq_raytracer_amd/csrc/hrt_launch_plan.h (what
// hrt_kernels.hip's launch wrappers and hrt_api.cpp run) compiled as plain C++, for tests/test_launch_plan.py
// to compare with a restatement of the rules.
//
// Cases on stdin, one per line; one JSON line per case:
//   t requested n_tris cam_list_capacity num_meshes max_bounces nodes entries wq_nodes wq_nodes_bfs sah_milli
//     bvh_n_nodes bvh_n_prims bvh_n_meshes wq_n_nodes wq_width max_leaf node_r lds_nodes_opt ncap_req tcap_req
//       the trace plan, the resolved kernel's traits and fit, every query method's plan, and wq_l2_plan
//       without the scene's presence flags and requests (what hrt_debug_wq_l2_plan exports)
//   s tiles n_frames num_cus split_factor_request
//       the heavy-tile rule: pair_split, plan_waves and plan_factor4 with and without it
#include <cstdio>
#include <cstdlib>

#include "hrt_launch_plan.h"

int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    long long v[20] = {0};
    char kind = 0;
    int used = 0, n = 0;
    if (std::sscanf(line, " %c%n", &kind, &used) != 1) continue;
    for (char* at = line + used; n < 20; ++n) {
      char* end;
      v[n] = std::strtoll(at, &end, 10);
      if (end == at) break;
      at = end;
    }
    if (kind == 's' && n == 4) {
      const uint32_t tiles = (uint32_t)v[0], frames = (uint32_t)v[1], cus = (uint32_t)v[2];
      const hrt::SplitFactor pair = hrt::pair_split(tiles, frames, cus, (int32_t)v[3]), plain{(int32_t)v[3], 0u};
      const uint32_t waves = hrt::plan_waves(cus, frames);
      std::printf("{\"factor\": %d, \"factor4\": %u, \"waves\": %u, \"pair_factor4\": %u, \"plain_factor4\": %u}\n",
                  pair.factor, pair.factor4, waves, hrt::plan_factor4(tiles, waves, pair),
                  hrt::plan_factor4(tiles, waves, plain));
    } else if (kind == 't' && n == 20) {
      const hrt::PlanScene s{(uint32_t)v[1],  (uint32_t)v[2],  (int32_t)v[3],   (int32_t)v[4],   v[5] != 0,
                             v[6] != 0,       v[7] != 0,       v[8] != 0,       (uint32_t)v[9],  (uint32_t)v[10],
                             (uint32_t)v[11], (uint32_t)v[12], (uint32_t)v[13], (uint32_t)v[14], (uint32_t)v[15],
                             (uint32_t)v[16], (int32_t)v[17],  (uint32_t)v[18], (uint32_t)v[19]};
      const hrt::LaunchPlan p = hrt::plan_trace(s, (int)v[0]);
      const hrt::KernelTraits& t = hrt::kernel_traits(p.kernel);
      std::printf("{\"kernel\": %d, \"block\": %u, \"groups\": %u, \"lds\": %zu, \"ncap\": %u, \"tcap\": %u, \"lnodes\": %u, "
                  "\"split_k\": %u, \"sec_batch\": %u, \"fits\": %d, \"persistent\": %d, \"lists\": %d, \"sky\": %d, "
                  "\"pairs\": %d, \"query\": [",
                  p.kernel, p.block, p.groups_per_cu, p.lds_bytes, p.wq_ncap, p.wq_tcap, p.wq_lds_nodes, p.split_k,
                  p.sec_batch, (int)hrt::kernel_fits(s, p.kernel), (int)t.persistent, (int)t.camera_lists,
                  (int)t.sky_lane, (int)t.pair_traversal);
      for (int m = HRT_QUERY_AUTO; m <= HRT_QUERY_PAIRS; ++m) {
        const hrt::QueryPlan q = hrt::plan_query(s, m);
        std::printf("%s[%d, %zu, %u, %u]", m ? ", " : "", q.method, q.lds_bytes, q.wq_ncap, q.wq_tcap);
      }
      uint32_t l2[4];
      hrt::wq_l2_plan(s.bvh_wq_n_nodes, s.bvh_wq_width, s.bvh_max_leaf, s.wq_lds_nodes_opt, 0u, 0u, l2);
      std::printf("], \"l2\": [%u, %u, %u, %u]}\n", l2[0], l2[1], l2[2], l2[3]);
    } else {
      std::fprintf(stderr, "bad case: %s", line);
      return 2;
    }
  }
  return 0;
}
