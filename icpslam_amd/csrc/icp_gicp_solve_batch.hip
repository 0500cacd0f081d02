// icp_gicp_solve_batch.hip -- several runs of the device solver in one launch: gicp_solve_batch_kernel.  The solver itself:
// icp_gicp_solve_device.h.
#include "icp_gicp_solve_device.h"

namespace icpgpu {
namespace {

// Several runs in ONE launch (icpgpu_align_batch in GICP mode): run = blockIdx.y, its own workgroups 0 .. workers - 1 (the
// others leave at once), its own slots, mailbox and numbers -- the runs share nothing but the launch.  Why: the runtime puts
// streams on four hardware queues and kernels that share a queue run one after the other, so with one resident solver kernel
// per run and outer iteration no more than four registrations ever solved at the same time (1.7k pairs/s whatever the
// scheduler, round 5: profiles/r05_gicp_batch.txt); one launch for all the runs that are ready lifts that.  Any placement
// (fine-grained slots): the one-XCD variant's placement trick does not compose with blockIdx.y.
struct GicpSolveBatchArgs {
  GicpSolveArgs a[kGicpSolveBatchMax];
};
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gicp_solve_batch_kernel(GicpSolveBatchArgs B) {
  const GicpSolveArgs& A = B.a[blockIdx.y];
  if ((int)blockIdx.x >= A.workers) return;
  gicp_solve_body<true, false>(A, (int)blockIdx.x, A.workers);
}

}  // namespace

hipError_t launch_gicp_solve_batch(const GicpSolveItem* items, int n, int max_inner, double gradient_tol, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (n > kGicpSolveBatchMax) return hipErrorInvalidValue;
  GicpSolveBatchArgs B;
  int max_blocks = 0;
  for (int k = 0; k < n; ++k) {
    const GicpSolveItem& it = items[k];
    if ((long long)it.blocks * 1024 < it.n_s) return hipErrorInvalidValue;  // resident shares only (the caller launches the others singly)
    B.a[k] = gicp_solve_args(it.blocks, it.src, it.n_s, it.tgt, it.keys, it.thr, it.base, it.guess, it.maha6, it.x0, it.slots, it.host_out, it.seq0,
                             max_inner, gradient_tol);
    max_blocks = it.blocks > max_blocks ? it.blocks : max_blocks;
  }
  for (int k = n; k < kGicpSolveBatchMax; ++k) B.a[k] = B.a[0];
  hipLaunchKernelGGL(gicp_solve_batch_kernel, dim3(max_blocks, n), dim3(256), 0, stream, B);
  return hipGetLastError();
}

}  // namespace icpgpu
