// icp_batch_plan.h -- the shape of one icpgpu_align_batch call: how many host threads, how many pairs each keeps in flight, and (for
// the lock-step path) how many groups each leads.  ONE definition, pure arithmetic over integers: no HIP, no environment, no
// context -- icpgpu_batch.cpp reads the switches and the CPUs and hands the numbers in.
//
// Point-to-point ICP: T host threads, each driving K worker contexts (own stream, scratch, grid, mailbox) ROUND-ROBIN --
// it polls the mailboxes of its contexts and does the host's share of an iteration (3x3 SVD, convergence test, next launch)
// for whichever has answered, so the kernels of K alignments are in flight per thread and nobody blocks on one result.
// T x K = 8 alignments in flight (a 50k-point sweep fills less than half of the chip), T from the CPUs this process may
// use: 4 x 2 on an unshared 16-CPU box, 2 x 4 when eight ranks share it.  GICP: one alignment per thread (its BFGS loop is
// a blocking host loop), T threads.  Every pair is solved exactly as icpgpu_align would solve it.
#pragma once
#include <algorithm>
#include <cstddef>

namespace icpgpu_impl {

struct BatchPlan {
  bool gicp = false;       // the method is GICP (else point-to-point)
  bool gicp_runs = false;  // GICP as resumable runs whose solvers leave in combined launches (else: a blocking host loop per run)
  bool lockstep = false;   // point-to-point in lock-step groups (else: the round-robin scheduler)
  size_t n_threads = 1;    // host threads
  size_t depth = 1;        // lock-step: pairs per group; otherwise: runs per thread
  size_t groups_per_thread = 1;
  size_t per_thread() const { return groups_per_thread * depth; }  // worker contexts of one thread
  size_t n_ctx() const { return n_threads * per_thread(); }
  // lock-step: one stream per group.  GICP runs: four streams per thread, created in a row = one per hardware queue: the combined
  // solver launches on the first, the runs' short kernels spread over the others.
  size_t streams_wanted() const { return lockstep ? n_threads * groups_per_thread : (gicp_runs ? 4 * n_threads : 0); }
};

// The most host threads a batch of this kind takes from the CPUs (an explicit thread count is not capped).
// GICP: resumable runs leave the host free (two threads x four runs measured 1.72k pairs/s on 13k-point clouds, one x eight 1.6-1.7k,
// eight x one 1.5k: profiles/r05_gicp_batch.txt); without the device solver every run is a blocking host loop and wants its own thread
inline size_t batch_thread_cap(bool gicp, bool gicp_runs) { return gicp ? (gicp_runs ? 2 : 8) : 4; }

// threads: what the switches or the CPUs give (>= 1); depth_override / groups_override: ICPGPU_BATCH_DEPTH / ICPGPU_BATCH_GROUPS as
// integers >= 1, 0 = not set; lockstep_max: the most pairs a lock-step launch takes (kBatchMax); server_workers: kMaxServerWorkers.
inline BatchPlan batch_plan(bool gicp, bool gicp_runs, bool lockstep, size_t n_pairs, size_t threads, size_t depth_override,
                            size_t groups_override, size_t lockstep_max, size_t server_workers) {
  BatchPlan p;
  p.gicp = gicp;
  p.gicp_runs = gicp_runs;
  p.lockstep = lockstep;
  size_t n_threads = threads, depth = 1;
  if (!gicp) {
    if (depth_override) depth = depth_override;
    else depth = lockstep ? 8 : std::max<size_t>(2, (8 + n_threads - 1) / n_threads);
    if (lockstep) depth = std::min<size_t>(depth, lockstep_max);
  } else {
    // GICP: kGicpRunsInFlight resumable runs over all threads (each keeps its solver's workgroups resident: eight of them, one
    // per XCD, is what the chip holds with room for everybody's searches -- kMaxServerWorkers); ICPGPU_BATCH_DEPTH = runs per thread
    if (depth_override) depth = depth_override;
    else if (gicp_runs) depth = std::max<size_t>(1, (16 + n_threads - 1) / n_threads);  // 16 runs in flight: their solvers leave in combined launches
    else depth = std::max<size_t>(1, (server_workers + n_threads - 1) / n_threads);
  }
  n_threads = std::min(n_threads, n_pairs);
  depth = std::min(depth, (n_pairs + n_threads - 1) / n_threads);
  // lock-step: groups in flight on the GPU = n_threads x groups_per_thread, eight by default whatever the CPUs (a 50k-point
  // group's sweep leaves the chip idle in its tail; measured at config 4's shape, 64 pairs: profiles/r05_batch_groups.txt).
  // ICPGPU_BATCH_GROUPS sets the total.
  size_t groups_per_thread = 1;
  if (lockstep) {
    size_t total = groups_override ? groups_override : 8;
    total = std::min(total, (n_pairs + depth - 1) / depth);
    n_threads = std::min(n_threads, std::max<size_t>(1, total));
    groups_per_thread = std::max<size_t>(1, (total + n_threads - 1) / n_threads);
  }
  p.n_threads = n_threads;
  p.depth = depth;
  p.groups_per_thread = groups_per_thread;
  return p;
}

}  // namespace icpgpu_impl
