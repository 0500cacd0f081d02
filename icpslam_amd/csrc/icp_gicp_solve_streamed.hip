// icp_gicp_solve_streamed.hip -- the device solver's kernel for shares larger than one quad per lane, streamed from memory at
// every evaluation: gicp_solve_kernel<false, false>.  The solver itself: icp_gicp_solve_device.h; launch_gicp_solve forwards here.
#include "icp_gicp_solve_device.h"

namespace icpgpu {

hipError_t launch_gicp_solve_streamed(int blocks, const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                                      const Xform& base, const float guess[16], const double* maha6, const double x0[6],
                                      unsigned long long* slots, unsigned long long* host_out, unsigned long long seq0, int max_inner,
                                      double gradient_tol, hipStream_t stream) {
  const GicpSolveArgs A = gicp_solve_args(blocks, src, n_s, tgt, keys, thr, base, guess, maha6, x0, slots, host_out, seq0, max_inner, gradient_tol);
  hipLaunchKernelGGL((gicp_solve_kernel<false, false>), dim3(blocks), dim3(256), 0, stream, A);
  return hipGetLastError();
}

}  // namespace icpgpu
