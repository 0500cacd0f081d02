// icpgpu_batch.cpp -- icpgpu_align_batch: many independent scan pairs through one context (BASELINE configs 4 / 5).
// The call's shape is icp_batch_plan.h's; this unit provisions it (worker contexts, their buffers, the groups' streams), starts the
// host threads and gives each to one of three drivers: GICP's resumable runs, the point-to-point lock-step groups
// (icpgpu_batch_lockstep.cpp) or the point-to-point round-robin scheduler.
#include "icp_batch.h"


namespace icpgpu_impl {

// The buffers a batch worker will need for pairs of up to ns x nt points, allocated BEFORE the batch runs (by the threads that
// create the workers, side by side) instead of at the worker's first pair: a worker's first use is a dozen hipMallocs in the
// middle of a running batch, and with 64 workers dealt pairs dynamically some of them meet their first pair only in the second,
// third or fifth call of a process (traced in round 5: every such call took 17-20 ms instead of 12.5).
static int presize_batch_worker(icpgpu_ctx* w, size_t ns, size_t nt, size_t table_cells) {
  if (w->batch_presized_src >= ns && w->batch_presized_tgt >= nt && w->batch_presized_cells >= table_cells) return ICPGPU_OK;
  int rc = ICPGPU_OK;
  auto need = [&](DeviceBuf& b, size_t bytes) { if (!rc && bytes) rc = ensure(w, b, bytes); };
  if (w->src.buf.external) w->src.buf = DeviceBuf{};
  if (w->tgt.buf.external) w->tgt.buf = DeviceBuf{};
  need(w->src.buf, ns * sizeof(float4));
  need(w->tgt.buf, nt * sizeof(float4));
  need(w->keys, ns * sizeof(unsigned long long));
  need(w->prev.buf, ns * sizeof(unsigned int));
  need(w->partials, (size_t)std::max(grid_search_blocks((int)ns), kMaxReduceBlocks) * kReduceTerms * sizeof(double));
  GridIndex& G = w->grid;
  need(G.ints, (6 + kGridStatInts) * sizeof(int));
  need(G.cell_of_point, nt * sizeof(int));
  need(G.rank, nt * sizeof(int));
  need(G.sorted, nt * sizeof(float4));
  need(G.unmatched, (ns + 1) * sizeof(int));
  if (table_cells) {
    const size_t cells = std::min<size_t>(table_cells + table_cells / 4, (size_t)kMaxGridCells + 1);
    need(G.cell_start, cells * sizeof(int));
    need(G.block_sums, (cells / kScanItems + 2) * sizeof(int));
  }
  if (!rc) {
    w->batch_presized_src = std::max(w->batch_presized_src, ns);
    w->batch_presized_tgt = std::max(w->batch_presized_tgt, nt);
    w->batch_presized_cells = std::max(w->batch_presized_cells, table_cells);
  }
  return rc;
}

// CPUs this process may use: the affinity mask, capped by the cgroup CPU quota (the GPU boxes grant 16 of 256 CPUs).
static int usable_cpus() {
  int n = (int)std::thread::hardware_concurrency();
  if (n < 1) n = 1;
#if defined(__linux__)
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min(n, std::max(1, CPU_COUNT(&set)));
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
    char q[64];
    long long period = 0;
    if (std::fscanf(f, "%63s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0)
      n = std::min(n, std::max(1, (int)(std::atoll(q) / period)));
    std::fclose(f);
  } else if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
    long long quota = -1, period = 0;
    if (std::fscanf(g, "%lld", &quota) != 1) quota = -1;
    std::fclose(g);
    if (FILE* h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (std::fscanf(h, "%lld", &period) != 1) period = 0;
      std::fclose(h);
    }
    if (quota > 0 && period > 0) n = std::min(n, std::max(1, (int)(quota / period)));
  }
#endif
  return n;
}

// Host threads of a batch: every one of them spins (on mailboxes, or inside a BFGS run), so there must be no more of them
// than CPUs -- across ALL the processes of the job: one process per GPU is the deployment (LOCAL_WORLD_SIZE, set by
// torch.distributed.run, says how many share this host's CPUs) -- and all the batch drivers inside THIS process that share its
// CPUs with this context's batch (c->host_share, icpgpu::set_ctx_host_share below).  ICPGPU_BATCH_THREADS overrides.
static size_t batch_threads(const icpgpu_ctx* c, size_t cap) {
  size_t t = 0;
  if (const char* v = std::getenv("ICPGPU_BATCH_THREADS")) t = (size_t)std::max(0, std::atoi(v));
  else if (const char* w = ICPGPU_DEV_ENV("ICPGPU_BATCH_WORKERS")) t = (size_t)std::max(0, std::atoi(w));  // round-1 name
  if (t == 0) {
    int local = 1;
    if (const char* l = std::getenv("LOCAL_WORLD_SIZE")) local = std::max(1, std::atoi(l));
    local *= c->host_share;
    t = (size_t)std::max(1, usable_cpus() / local);
    t = std::min(t, cap);
  }
  return std::max<size_t>(1, t);
}

static size_t env_at_least_one(const char* name) {  // 0: not set
  const char* v = std::getenv(name);
  return v ? (size_t)std::max(1, std::atoi(v)) : 0;
}

// Items first .. last - 1 made by n_makers threads side by side (maker m: first + m, first + m + n_makers, ...), joined; make(i) is
// the item's return code.  Handed back: the first failure in index order (index == last: none).
struct MakeFailure {
  size_t index;
  int rc;
};
template <class Make>
static MakeFailure make_side_by_side(size_t first, size_t last, size_t n_makers, Make&& make) {
  std::vector<int> rc(last - first, 0);
  std::vector<std::thread> makers;
  for (size_t m = 0; m < n_makers; ++m)
    makers.emplace_back([&, m] {
      for (size_t i = first + m; i < last; i += n_makers) rc[i - first] = make(i);
    });
  for (auto& th : makers) th.join();
  for (size_t i = first; i < last; ++i)
    if (rc[i - first]) return {i, rc[i - first]};
  return {last, 0};
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Worker contexts are created on first use, by the batch threads in parallel (a context is a stream, two hundred events and a
// dozen pinned / fine-grained / device allocations: ~1 ms, and a batch wants up to 64 of them -- created one after the other by
// the calling thread they were most of the first call's time)
static int provide_workers(icpgpu_ctx* c, const BatchPlan& plan, double& create_ms) {
  const size_t n_ctx = plan.n_ctx(), have = c->workers.size();
  if (have >= n_ctx) return ICPGPU_OK;
  const auto t_create = std::chrono::steady_clock::now();
  c->workers.resize(n_ctx, nullptr);
  std::vector<std::string> create_msg(n_ctx);  // (icpgpu_last_error(nullptr) is per thread: taken where it was set)
  const size_t n_makers = std::min<size_t>(std::max<size_t>(1, plan.n_threads), n_ctx - have);
  const bool with_stream = !(plan.lockstep || plan.gicp_runs);  // (lock-step workers run on their group's stream, GICP runs on their thread's)
  const MakeFailure bad = make_side_by_side(have, n_ctx, n_makers, [&](size_t i) {
    icpgpu_ctx* w = nullptr;
    const int rc = create_context(&w, c->device, with_stream);
    if (rc == ICPGPU_OK) w->shared_table_cells = &c->batch_table_cells;
    else create_msg[i] = icpgpu_last_error(nullptr);
    c->workers[i] = w;
    return rc;
  });
  if (bad.index < n_ctx) {
    for (size_t k = have; k < n_ctx; ++k)
      if (c->workers[k]) icpgpu_destroy(c->workers[k]);
    c->workers.resize(have);
    return fail(c, bad.rc, "align_batch: worker context: %s", create_msg[bad.index].c_str());
  }
  create_ms += ms_since(t_create);
  return ICPGPU_OK;
}

// lock-step: every worker's buffers for this batch's largest clouds (nothing to do once they are there)
static int presize_workers(icpgpu_ctx* c, const BatchPlan& plan, size_t n_pairs, const size_t* n_src, const size_t* n_tgt, double& create_ms) {
  const size_t n_ctx = plan.n_ctx();
  size_t ns_max = 0, nt_max = 0;
  for (size_t k = 0; k < n_pairs; ++k) {
    ns_max = std::max(ns_max, n_src[k]);
    nt_max = std::max(nt_max, n_tgt[k]);
  }
  const size_t cells = c->batch_table_cells.load(std::memory_order_relaxed);
  bool all_there = true;
  for (size_t i = 0; i < n_ctx && all_there; ++i)
    all_there = c->workers[i]->batch_presized_src >= ns_max && c->workers[i]->batch_presized_tgt >= nt_max && c->workers[i]->batch_presized_cells >= cells;
  if (all_there) return ICPGPU_OK;
  const auto t_pre = std::chrono::steady_clock::now();
  const size_t n_makers = std::min<size_t>(std::max<size_t>(1, plan.n_threads), n_ctx);
  const MakeFailure bad = make_side_by_side(0, n_ctx, n_makers, [&](size_t i) {
    if (hipSetDevice(c->device) != hipSuccess)  // (reported through the worker the maker was about to size)
      return fail(c->workers[i], ICPGPU_ERR_HIP, "hipSetDevice failed in a batch maker thread");
    return presize_batch_worker(c->workers[i], ns_max, nt_max, cells);
  });
  if (bad.index < n_ctx) return fail(c, bad.rc, "align_batch: worker buffers: %s", c->workers[bad.index]->err.c_str());
  create_ms += ms_since(t_pre);
  return ICPGPU_OK;
}

// The groups' streams are created HERE, one after the other: the runtime spreads streams over its (four) hardware queues in
// creation order, and kernels of streams that share a hardware queue do not overlap.  Until round 5 a group ran on its lead
// worker's stream -- the (g x depth)-th stream the context created -- so that with a depth of 8 (or 4) EVERY group sat on the
// same hardware queue and the groups' sweeps ran one after the other: 4.1-4.5k pairs/s at config 4's shape where depths of
// 5 or 7 reached 5.1-5.5k (rocprofv3 kernel trace: 2 queues in use, mostly one search kernel at a time, against 4 queues and
// 2-4 kernels; profiles/r05_batch_groups.txt).
// (hipStreamCreate is 3-4 ms apiece on this runtime when called in a row -- scripts/probes/create_probe.cpp -- and well under a
//  millisecond each from several threads at once: the missing streams are created side by side, then appended in order)
static int provide_streams(icpgpu_ctx* c, const BatchPlan& plan) {
  const size_t have = c->group_streams.size(), want = plan.streams_wanted();
  if (have >= want) return ICPGPU_OK;
  std::vector<hipStream_t> fresh(want - have, nullptr);
  const MakeFailure bad = make_side_by_side(0, fresh.size(), fresh.size(), [&](size_t k) {  // (a maker per stream; rc: the hipError_t)
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&fresh[k], hipStreamNonBlocking);
    return (int)e;
  });
  if (bad.index < fresh.size()) {
    for (hipStream_t st : fresh)
      if (st) (void)hipStreamDestroy(st);
    return fail(c, ICPGPU_ERR_HIP, "align_batch: hipStreamCreate: %s", hipGetErrorString((hipError_t)bad.rc));
  }
  for (hipStream_t st : fresh) c->group_streams.push_back(st);
  return ICPGPU_OK;
}

// ---- GICP: `depth` resumable runs per thread ---------------------------------------------------------------------------------------
// Round-robin (GicpRun, icpgpu_gicp.cpp): the thread queues a run's next stage when
// its awaited result has arrived and looks at the others meanwhile -- until round 5 it was ONE blocking alignment per
// thread, its host spinning through every inner minimisation.  A run that cannot be resumable (no device solver on its
// context, or the solver gave up) is one blocking alignment inside its step.
// With the device solver (gicp_runs): the solvers of the runs that are ready go out TOGETHER, one gicp_solve_batch_kernel
// launch on the thread's solve stream behind the runs' events -- a resident solver kernel per run would hold a hardware
// queue each, four registrations at most solving at any time.  The runs' short kernels (index builds, covariances, searches,
// fitness) go to three work streams, created right behind the solve stream and therefore on the three OTHER hardware queues:
// nothing short ever waits behind a solver.  (One work stream for all runs was tried first: every run's next step then
// queued behind every other run's covariance pass -- 0.5-1.1k pairs/s instead of 1.7k.)
namespace {
struct GicpRuns {
  BatchJob& job;
  size_t t;
  icpgpu_ctx* const* ws;
  std::vector<GicpRun> runs;
  std::vector<size_t> pair_of;
  // Two solve streams, two work streams.  A solve stream takes a new launch only when the runs of its last one have all
  // answered (launches on one stream run one after the other: a launch per ready run, issued at once, put every run behind
  // every other -- 0.57k pairs/s); meanwhile the runs that become ready collect and leave together.
  hipStream_t work_stream[2] = {nullptr, nullptr}, solve_stream[2] = {nullptr, nullptr};
  std::vector<hipStream_t> own;
  std::vector<int> solving_on;  // which solve stream a run's solver is on (-1: none)
  int blocks_on[2] = {0, 0};    // solver workgroups the launch in flight on each solve stream holds
  GicpRuns(BatchJob& j, size_t thread)
      : job(j), t(thread), ws(j.workers_of(thread)), runs(j.plan.depth), pair_of(j.plan.depth, 0), own(j.plan.depth, nullptr), solving_on(j.plan.depth, -1) {
    if (!job.plan.gicp_runs) return;
    for (int k = 0; k < 2; ++k) solve_stream[k] = job.c->group_streams[4 * t + k];
    for (int k = 0; k < 2; ++k) work_stream[k] = job.c->group_streams[4 * t + 2 + k];
    for (size_t s = 0; s < runs.size(); ++s) {
      own[s] = ws[s]->stream;
      ws[s]->stream = work_stream[s % 2];
    }
  }
  ~GicpRuns() {  // (RestoreStreams) whatever way the thread leaves: nothing of it in flight, the workers get their own streams back
    if (!solve_stream[0]) return;
    for (int k = 0; k < 2; ++k) (void)hipStreamSynchronize(solve_stream[k]);
    for (int k = 0; k < 2; ++k) (void)hipStreamSynchronize(work_stream[k]);
    for (size_t i = 0; i < own.size(); ++i) ws[i]->stream = own[i];
  }
  int launch_ready_solvers(int ss, bool& progressed);
};

// the solvers of every run that is ready: one launch, on solve stream `ss` if it is idle.  < 0: failed (the thread's error is set)
int GicpRuns::launch_ready_solvers(int ss, bool& progressed) {
  const size_t depth = runs.size();
  bool busy = false, other_busy = false;
  for (size_t s = 0; s < depth; ++s) {
    if (solving_on[s] >= 0 && runs[s].phase != GicpRun::Solve) solving_on[s] = -1;  // (answered, or gave up)
    busy = busy || solving_on[s] == ss;
    other_busy = other_busy || solving_on[s] == 1 - ss;
  }
  if (busy) return 0;
  blocks_on[ss] = 0;
  if (!other_busy) blocks_on[1 - ss] = 0;
  GicpSolveItem items[kGicpSolveBatchMax];
  size_t who[kGicpSolveBatchMax];
  int n_ready = 0, blocks_sum = 0;
  // (a solver workgroup takes a CU's one-wave-per-SIMD slot: the workgroups resident over BOTH solve streams of ALL threads
  //  together stay below the chip's 256 CUs, or a run's workgroups would spin waiting for peers that have no CU yet.  Until
  //  round 6 the cap was applied per launch, and two launches of a thread could hold ~2 x 240 / n_threads between them.)
  const int blocks_cap = std::max(1, 240 / (int)job.plan.n_threads) - blocks_on[1 - ss];
  for (size_t s = 0; s < depth && n_ready < kGicpSolveBatchMax; ++s)
    if (runs[s].phase == GicpRun::WantSolve && ((n_ready == 0 && !other_busy) || blocks_sum + runs[s].item.blocks <= blocks_cap)) {
      items[n_ready] = runs[s].item;
      blocks_sum += runs[s].item.blocks;
      who[n_ready++] = s;
    }
  if (!n_ready) return 0;
  hipError_t e = hipSuccess;
  for (int k = 0; k < n_ready && e == hipSuccess; ++k) {  // behind each run's own search and Mahalanobis kernels
    icpgpu_ctx* w = ws[who[k]];
    e = hipEventRecord(w->ev[0], w->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(solve_stream[ss], w->ev[0], 0);
  }
  if (e == hipSuccess) e = launch_gicp_solve_batch(items, n_ready, 20, 1e-2, solve_stream[ss]);
  if (e != hipSuccess) {
    fail(ws[who[0]], ICPGPU_ERR_HIP, "GICP batch: solver launch: %s", hipGetErrorString(e));
    job.failed(t, ICPGPU_ERR_HIP, pair_of[who[0]], ws[who[0]]);
    return -1;
  }
  for (int k = 0; k < n_ready; ++k) {
    gicp_run_solver_launched(ws[who[k]], runs[who[k]], solve_stream[ss]);
    solving_on[who[k]] = ss;
  }
  blocks_on[ss] = blocks_sum;
  progressed = true;
  return 0;
}
}  // namespace

static void run_gicp_runs(BatchJob& job, size_t t) {
  GicpRuns R(job, t);
  const bool combine = job.plan.gicp_runs;
  for (;;) {
    bool progressed = false;
    size_t in_flight = 0;
    for (size_t s = 0; s < R.runs.size(); ++s) {
      GicpRun& r = R.runs[s];
      icpgpu_ctx* w = R.ws[s];
      if (r.phase == GicpRun::Idle || r.phase == GicpRun::Done) {
        size_t k = 0;
        if (!job.claim(k)) continue;
        R.pair_of[s] = k;
        int rc = job.load_pair(w, k, /*sync=*/false);
        if (!rc) rc = gicp_run_begin(w, r, job.want_fitness, &job.results[k], combine);
        if (rc) return job.failed(t, rc, k, w);
        progressed = true;
      } else {
        const int st = gicp_run_step(w, r);
        if (st < 0) return job.failed(t, st, R.pair_of[s], w);
        progressed = progressed || st > 0;
      }
      if (r.phase != GicpRun::Done) ++in_flight;
    }
    if (in_flight == 0 && (job.exhausted() || job.abort.load())) return;
    for (int ss = 0; combine && ss < 2; ++ss)
      if (R.launch_ready_solvers(ss, progressed)) return;
#if defined(__x86_64__)
    if (!progressed) __builtin_ia32_pause();
#endif
  }
}

// ---- point-to-point, round-robin (ICPGPU_BATCH_LOCKSTEP=0: the scheduler of round 2) ---------------------------------------------------
// Every worker on its own stream; the thread polls their mailboxes and does the host's share of an iteration for whichever has answered.
static void run_round_robin(BatchJob& job, size_t t) {
  icpgpu_ctx* const* ws = job.workers_of(t);
  const size_t depth = job.plan.depth;
  std::vector<P2PRun> runs(depth);
  std::vector<size_t> pair_of(depth, 0);
  for (unsigned idle_spins = 0;;) {
    bool progressed = false;
    size_t in_flight = 0;
    for (size_t s = 0; s < depth; ++s) {
      P2PRun& r = runs[s];
      icpgpu_ctx* w = ws[s];
      if (r.phase == P2PRun::Idle || r.phase == P2PRun::Done) {
        size_t k = 0;
        if (!job.claim(k)) continue;
        pair_of[s] = k;
        int rc = job.load_pair(w, k);
        if (!rc) rc = p2p_begin(w, r, nullptr, nullptr, job.want_fitness, &job.results[k]);
        if (rc) return job.failed(t, rc, k, w);
        progressed = true;
      } else if (sweep_ready(w, r.ticket)) {
        const int rc = p2p_advance(w, r);
        if (rc) return job.failed(t, rc, pair_of[s], w);
        progressed = true;
      }
      if (r.phase != P2PRun::Done) ++in_flight;
    }
    if (in_flight == 0 && (job.exhausted() || job.abort.load())) return;
    if (progressed) {
      idle_spins = 0;
      continue;
    }
    if ((++idle_spins & 0x3FFu) == 0)  // nothing moved for a while: every awaited run's own stream, and the clock
      for (size_t s = 0; s < depth; ++s) {
        if (runs[s].phase != P2PRun::Iterating && runs[s].phase != P2PRun::Fitness) continue;
        if (batch_stall_look(ws[s], {ws[s]->stream}, runs[s].t_issue)) return job.failed(t, ICPGPU_ERR_HIP, pair_of[s], ws[s]);
      }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
}

// one host thread of the call: its workers' settings, then the driver the plan names
static void batch_thread(BatchJob& job, size_t t) {
  icpgpu_ctx* c = job.c;
  const BatchPlan& plan = job.plan;
  if (hipSetDevice(c->device) != hipSuccess) {
    job.errors[t].code = ICPGPU_ERR_HIP;
    job.errors[t].msg = "hipSetDevice failed in a batch thread";
    job.abort.store(true);
    return;
  }
  icpgpu_ctx* const* ws = job.workers_of(t);
  const size_t in_flight = plan.n_threads * (plan.gicp ? plan.depth : 1);
  for (size_t s = 0; s < plan.per_thread(); ++s) {
    ws[s]->params = c->params;
    ws[s]->nn_variant = c->nn_variant;
    // Every GICP worker's BFGS runs keep its workgroups resident and a host thread spinning.  8 workers fit the chip
    // with room for everybody's searches; 16 were measured 5x SLOWER than single launches (servers wait for slots other
    // servers hold until their 50 ms patience runs out).
    ws[s]->gicp_server_allowed = in_flight <= 2 * kMaxServerWorkers;
    // ... and each worker's evaluations get their share of the ~512 workgroups of that size the chip holds at once (64
    // apiece for 8 workers, as measured in round 1; a lone alignment uses up to 256)
    ws[s]->gicp_blocks_most = std::max(16, std::min(kGicpDirectBlocks, 512 / (int)std::max<size_t>(1, in_flight)));
  }
  if (!plan.lockstep && !plan.gicp_runs)  // these paths run every worker on its own stream
    for (size_t s = 0; s < plan.per_thread(); ++s)
      if (ensure_stream(ws[s])) return job.failed(t, ICPGPU_ERR_HIP, 0, ws[s]);
  if (plan.gicp) return run_gicp_runs(job, t);
  if (plan.lockstep) return run_lockstep_groups(job, t);
  return run_round_robin(job, t);
}

// the workers' kernel accounting goes into the parent's profile and starts over
static void fold_profile(icpgpu_profile& dst, icpgpu_profile& src) {
  static constexpr uint64_t icpgpu_profile::* counters[] = {
      &icpgpu_profile::nn_launches, &icpgpu_profile::nn_pairs, &icpgpu_profile::nn_bytes, &icpgpu_profile::reduce_launches, &icpgpu_profile::reduce_bytes,
      &icpgpu_profile::transform_launches, &icpgpu_profile::transform_bytes, &icpgpu_profile::iterations, &icpgpu_profile::aligns,
      &icpgpu_profile::grid_launches, &icpgpu_profile::grid_bytes, &icpgpu_profile::nn_timed, &icpgpu_profile::grid_timed, &icpgpu_profile::reduce_timed,
      &icpgpu_profile::grid_bounded, &icpgpu_profile::grid_builds, &icpgpu_profile::grid_fallback_points, &icpgpu_profile::voxel_launches,
      &icpgpu_profile::voxel_bytes, &icpgpu_profile::gicp_cov_launches, &icpgpu_profile::gicp_cost_launches, &icpgpu_profile::gicp_eval_corr,
      &icpgpu_profile::gicp_cov_points, &icpgpu_profile::targets_recognised, &icpgpu_profile::brute_bound_violations, &icpgpu_profile::gicp_device_solves,
      &icpgpu_profile::gicp_host_solves, &icpgpu_profile::gicp_quadratic_solves, &icpgpu_profile::sources_adopted, &icpgpu_profile::grid_adopted};
  static constexpr double icpgpu_profile::* milliseconds[] = {
      &icpgpu_profile::nn_ms, &icpgpu_profile::reduce_ms, &icpgpu_profile::transform_ms, &icpgpu_profile::grid_ms, &icpgpu_profile::grid_build_ms,
      &icpgpu_profile::voxel_ms, &icpgpu_profile::gicp_cov_ms, &icpgpu_profile::gicp_eval_ms};
  for (auto m : counters) dst.*m += src.*m;
  for (auto m : milliseconds) dst.*m += src.*m;
  if (src.brute_bound_worst > dst.brute_bound_worst) dst.brute_bound_worst = src.brute_bound_worst;
  std::memset(&src, 0, sizeof(src));
}

static int align_batch_impl(icpgpu_ctx* c, size_t n_pairs, const float* const* src, const size_t* n_src, const float* const* tgt,
                            const size_t* n_tgt, int want_fitness, icpgpu_result* results) {
  const bool gicp = c->params.method == ICPGPU_GICP;
  // Point-to-point batches run in LOCK-STEP (ICPGPU_BATCH_LOCKSTEP=0: the round-robin scheduler of round 2): a host thread
  // leads a group of `depth` pairs on ONE stream -- their index builds go through their host round trips together, and
  // every ICP iteration of the whole group is one search launch (pair = blockIdx.y, nn_quad_batch_kernel) + one final
  // reduction launch (17 x K workgroups) + K host solves, instead of K x (launch + reduce + poll): ~35 launches per K
  // pairs where there were ~35 per pair.  Two threads keep the GPU fed (one copies its next group in while the other's
  // group iterates); results are bit-identical to icpgpu_align's (same kernels' bodies, same workgroup -> point mapping).
  static const bool lockstep_on = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_BATCH_LOCKSTEP"); return !e || std::atoi(e) != 0; }();
  if (gicp) {
    const int grc = ensure_gicp_resources(c);
    if (grc) return grc;
  }
  const bool gicp_runs = gicp && (gicp_inner_quadratic(c) || (gicp_device_solver_mode() != 0 && c->gicp_device_ok));  // (quadratic runs need no device solver)
  BatchJob job;
  job.plan = batch_plan(gicp, gicp_runs, lockstep_on && !gicp, n_pairs, batch_threads(c, batch_thread_cap(gicp, gicp_runs)),
                        env_at_least_one("ICPGPU_BATCH_DEPTH"), env_at_least_one("ICPGPU_BATCH_GROUPS"), (size_t)kBatchMax, kMaxServerWorkers);
  const BatchPlan& plan = job.plan;
  double create_ms = 0.0;  // (the trace line's)
  int rc = provide_workers(c, plan, create_ms);
  if (!rc && plan.lockstep) rc = presize_workers(c, plan, n_pairs, n_src, n_tgt, create_ms);
  if (!rc) rc = provide_streams(c, plan);
  if (rc) return rc;
  job.c = c;
  job.n_pairs = n_pairs;
  job.src = src;
  job.n_src = n_src;
  job.tgt = tgt;
  job.n_tgt = n_tgt;
  job.want_fitness = want_fitness;
  job.results = results;
  job.errors.resize(plan.n_threads);
  job.t_call = std::chrono::steady_clock::now();
  std::vector<std::thread> threads;
  for (size_t t = 1; t < plan.n_threads; ++t) threads.emplace_back([&job, t] { batch_thread(job, t); });
  batch_thread(job, 0);
  for (auto& th : threads) th.join();
  for (size_t i = 0; i < plan.n_ctx(); ++i) fold_profile(c->prof, c->workers[i]->prof);
  {
    static const bool trace = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_BATCH_TRACE"); return e && std::atoi(e) != 0; }();
    if (trace)
      fprintf(stderr, "[icpgpu] batch trace: call of %zu pairs took %.2f ms (+ %.2f ms creating worker contexts); device allocations so far in this process: %llu, %.2f ms of host time\n", n_pairs,
              ms_since(job.t_call), create_ms, g_alloc_calls.load(), g_alloc_us.load() * 1e-3);
  }
  for (const ThreadError& e : job.errors)  // the first failure in thread order (each thread stops at its first)
    if (e.code != ICPGPU_OK) {
      c->err = "align_batch pair " + std::to_string(e.pair) + ": " + e.msg;
      return e.code;
    }
  return ICPGPU_OK;
}

}  // namespace icpgpu_impl

namespace icpgpu {
// batch drivers inside THIS process that share its CPUs with this context's batch (icpgpu_align_batch_multi: one per device;
// a property of the context, so that concurrent callers cannot overwrite each other's share)
void set_ctx_host_share(icpgpu_ctx* c, int peers) {
  if (c) c->host_share = peers < 1 ? 1 : peers;
}
}  // namespace icpgpu

extern "C" int icpgpu_align_batch(icpgpu_ctx* c, size_t n_pairs, const float* const* src, const size_t* n_src,
                                  const float* const* tgt, const size_t* n_tgt, int want_fitness, icpgpu_result* results) {
  ENTER(c);
  if (n_pairs && (!src || !n_src || !tgt || !n_tgt || !results)) return fail(c, ICPGPU_ERR_INVALID_ARG, "null argument");
  if (c->params.method == ICPGPU_P2PLANE) return fail(c, ICPGPU_ERR_UNSUPPORTED, "align_batch: the point-to-plane method has no batch path");
  if (c->params.method == ICPGPU_NDT) return fail(c, ICPGPU_ERR_UNSUPPORTED, "align_batch: the NDT method has no batch path");
  if (c->n_rejectors > 0) return fail(c, ICPGPU_ERR_UNSUPPORTED, "align_batch: correspondence rejectors have no batch path (the lock-step kernels fuse the reduction)");
  if (c->p2plane_symmetric) return fail(c, ICPGPU_ERR_UNSUPPORTED, "align_batch: the symmetric point-to-plane objective has no batch path");
  if (c->reciprocal) return fail(c, ICPGPU_ERR_UNSUPPORTED, "align_batch: reciprocal correspondences have no batch path (the lock-step kernels fuse the reduction)");
  if (n_pairs == 0) return ICPGPU_OK;
  if (c->abi_result == sizeof(icpgpu_result)) return align_batch_impl(c, n_pairs, src, n_src, tgt, n_tgt, want_fitness, results);
  // the caller's icpgpu_result has another length (include/icpgpu.h, ABI rule): its array has ITS stride
  std::vector<icpgpu_result> own(n_pairs);
  const int rc = align_batch_impl(c, n_pairs, src, n_src, tgt, n_tgt, want_fitness, own.data());
  unsigned char* out = reinterpret_cast<unsigned char*>(results);
  for (size_t k = 0; k < n_pairs; ++k) {
    std::memset(out + k * c->abi_result, 0, c->abi_result);
    std::memcpy(out + k * c->abi_result, &own[k], std::min(c->abi_result, sizeof(icpgpu_result)));
  }
  return rc;
}
