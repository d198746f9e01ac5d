// phase_batch_plan_test.cpp -- prints, for every kernel row of epq_raytracer_amd/csrc/hrt_launch_plan.h and both
// values of the scene's bvh_node_r, the row's two thresholds (KernelTraits), what size_kernel puts into the
// plan, and what a launch runs with for the requests on the command line (batch_threshold, as launch_trace
// resolves HRT_OPT_PRIMARY_BATCH / HRT_OPT_SECONDARY_BATCH); for tests/test_phase_batch_plan.py.
#include <cstdio>
#include <cstdlib>

#include "hrt_launch_plan.h"

int main(int argc, char** argv) {
  for (int k = 0; k < hrt::kNumKernels; ++k) {
    for (uint32_t node_r = 0; node_r < 2; ++node_r) {
      hrt::PlanScene s{};
      s.bvh_node_r = node_r;
      hrt::LaunchPlan plan;
      hrt::size_kernel(s, k, plan);  // (the thresholds are set whether or not this empty scene fits the row)
      const hrt::KernelTraits& t = hrt::kernel_traits(k);
      std::printf("{\"kernel\": %d, \"node_r\": %u, \"pairs\": %d, \"row\": [%u, %u, %u, %u], \"plan\": [%u, %u], \"resolved\": [",
                  k, node_r, (int)t.pair_traversal, t.sec_batch, t.sec_batch_node_r, t.prim_batch, t.prim_batch_node_r,
                  plan.sec_batch, plan.prim_batch);
      for (int i = 1; i < argc; ++i) {
        const uint32_t request = (uint32_t)std::strtoul(argv[i], nullptr, 10);
        std::printf("%s[%u, %u]", i > 1 ? ", " : "", hrt::batch_threshold(request, plan.sec_batch),
                    hrt::batch_threshold(request, plan.prim_batch));
      }
      std::printf("]}\n");
    }
  }
  return 0;
}
