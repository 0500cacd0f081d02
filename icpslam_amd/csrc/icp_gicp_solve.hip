// icp_gicp_solve.hip -- the device solver's single-run kernels whose correspondences stay in registers: gicp_solve_kernel<true, false>
// (any placement) and gicp_solve_kernel<true, true> (one XCD).  The solver itself: icp_gicp_solve_device.h.
#include "icp_gicp_solve_device.h"

namespace icpgpu {

// The device solver: one resident kernel per outer iteration (see gicp_solve_kernel).  `blocks` workgroups of 256 lanes, all
// co-resident; RESIDENT when every lane's share of the correspondences is one quad.
size_t gicp_solve_slot_bytes(int blocks) { return (size_t)2 * (size_t)blocks * kSolveGranules * 2 * sizeof(unsigned long long); }
int gicp_solve_out_granules() { return kSolveOut; }
int gicp_solve_local_blocks() { return kSolveLocalBlocks; }
hipError_t launch_gicp_solve(int blocks, const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                             const Xform& base, const float guess[16], const double* maha6, const double x0[6],
                             unsigned long long* slots, unsigned long long* host_out, unsigned long long seq0, int max_inner,
                             double gradient_tol, hipStream_t stream, unsigned long long* local_slots, unsigned long long* owner,
                             int xcc_want) {
  if ((long long)blocks * 1024 < n_s)  // not resident
    return launch_gicp_solve_streamed(blocks, src, n_s, tgt, keys, thr, base, guess, maha6, x0, slots, host_out, seq0, max_inner, gradient_tol, stream);
  GicpSolveArgs A = gicp_solve_args(blocks, src, n_s, tgt, keys, thr, base, guess, maha6, x0, slots, host_out, seq0, max_inner, gradient_tol);
  if (local_slots && owner && blocks <= kSolveLocalBlocks) {  // one XCD: up to 32 workgroups (one per CU of the XCD)
    A.slots = local_slots;
    A.xcc_want = xcc_want;
    A.owner = owner;
    hipLaunchKernelGGL((gicp_solve_kernel<true, true>), dim3(8 * blocks), dim3(256), 0, stream, A);
  } else {
    hipLaunchKernelGGL((gicp_solve_kernel<true, false>), dim3(blocks), dim3(256), 0, stream, A);
  }
  return hipGetLastError();
}

}  // namespace icpgpu
