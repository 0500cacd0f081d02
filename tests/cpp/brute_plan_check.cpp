// brute_plan_check.cpp -- icpslam_amd/csrc/icp_brute_plan.h on the host: the launch plan of the matrix-core brute-force kernels for
// a table of (n_q, n_t, num_cus) read from stdin, one line each, for the three shapes that ship: the f32 kernel's, the bf16
// kernel's and its bound-check shape.  tests/test_brute_plan_host.py holds every line to the Python restatement.
//   in:  n_q n_t num_cus
//   out: shape n_q n_t num_cus g tile block grid_x splits tgt_per_split
#include <cstdio>

#include "icp_brute_plan.h"

int main() {
  using namespace icpgpu;
  const struct { const char* name; MatrixNnShape shape; } shapes[] = {{"mfma", kMfmaShape}, {"bf16", kBf16Shape}, {"bf16-check", kBf16CheckShape}};
  int n_q, n_t, num_cus;
  while (scanf("%d %d %d", &n_q, &n_t, &num_cus) == 3) {
    for (const auto& s : shapes) {
      const MatrixNnPlan p = matrix_nn_plan(n_q, n_t, num_cus, s.shape, kMatrixNnWavesPerSimd);
      printf("%s %d %d %d %d %d %d %d %d %d\n", s.name, n_q, n_t, num_cus, p.g, p.tile, p.block, p.grid_x, p.splits, p.tgt_per_split);
    }
  }
  return 0;
}
