// icpgpu_batch_lockstep.cpp -- icpgpu_align_batch, point-to-point: a host thread's lock-step groups.
// A host thread leads `groups_per_thread` groups, each `depth` pairs on a stream of its own, as NON-BLOCKING state
// machines (fill -> index builds -> iterate): while one group's sweep is in flight the thread copies the next pair of
// another group in, takes that group's builds through a host round trip, or does its solves.  The number of groups in
// flight on the GPU is therefore decoupled from the number of CPUs the process may use (round 4: one group per thread,
// four threads at most -- 4.0k pairs/s at config 4's shape where eight such entries sharing the GPU reached 5.2k: the
// sweeps of one group leave the chip idle in their tails, more groups fill them).
#include "icp_batch.h"

namespace icpgpu_impl {
namespace {

struct Slot {
  icpgpu_ctx* w = nullptr;
  size_t pair = 0;
  P2PRun run;
  GridBuild gb;
  bool lock = false;       // iterates inside the group's lock-step launches (else: the single-pair state machine)
  bool wants = false;      // lock-step: its next gated sweep is due
  bool wants_fit = false;  // lock-step: its ungated fitness sweep is due
  bool waiting = false;    // lock-step: a sweep of it is in flight
  bool pack = false;
  unsigned int* prev = nullptr;
  bool awaited() const { return run.phase == P2PRun::Iterating || run.phase == P2PRun::Fitness; }
};

struct Group {
  enum Phase { Fill, Build, Iterate, Retired } phase = Fill;
  icpgpu_ctx* const* ws = nullptr;
  icpgpu_ctx* lead = nullptr;
  hipStream_t gstream = nullptr;  // copies, index builds, the table: the lead's own stream
  hipStream_t sstream = nullptr;  // the sweeps (search + reduction + the fitness tail): the same stream (see run_lockstep_groups)
  std::vector<hipStream_t> own;
  std::vector<Slot> slots;
  std::vector<BatchPair> table;
  size_t n_slots = 0, live = 0, cap = 0;  // cap: pairs the current fill takes (the thread's first one is small: see fill_step)
  unsigned idle_spins = 0, step_counter = 0;
  int timed_pairs = 0;  // pairs of the launch whose events are outstanding
  size_t index = 0;     // the group's number among all groups of the job
  bool filled_once = false;
  unsigned long long sync_seq = 0;  // Build: the number the group's posted marker carries once its stage has drained
  std::chrono::steady_clock::time_point bt0, bt1, bt2;
  ~Group() {  // whatever way the thread leaves: the workers get their own streams back, nothing of the group in flight
    if (sstream) (void)hipStreamSynchronize(sstream);
    if (gstream) (void)hipStreamSynchronize(gstream);
    for (size_t i = 0; i < own.size(); ++i) ws[i]->stream = own[i];
  }
};

bool stagger_on() { static const bool v = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_BATCH_STAGGER"); return !e || std::atoi(e) != 0; }(); return v; }
bool bt_on() { static const bool v = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_BATCH_TIMING"); return e && std::atoi(e) != 0; }(); return v; }
bool bt_trace() { static const bool v = [] { const char* e = ICPGPU_DEV_ENV("ICPGPU_BATCH_TRACE"); return e && std::atoi(e) != 0; }(); return v; }

// one host thread's view of the job, and (ICPGPU_BATCH_TIMING=1) what its groups spent where
struct Leader {
  BatchJob& job;
  size_t t;
  double bt_fill = 0, bt_build = 0, bt_iter = 0;
  size_t bt_groups = 0, bt_steps = 0;
  int bail(int rc, size_t k, icpgpu_ctx* w) {
    job.failed(t, rc, k, w);
    return -1;
  }
  ~Leader() {
    if (bt_on() && bt_groups)
      fprintf(stderr, "[icpgpu] batch thread %zu: %zu groups, %zu steps; per group: fill (H2D) %.3f ms, index builds %.3f ms, iterations + fitness %.3f ms\n", t,
              bt_groups, bt_steps, bt_fill / bt_groups, bt_build / bt_groups, bt_iter / bt_groups);
  }
};

// queue a marker behind everything the group's stream holds: the stage has drained once the mailbox carries its number
int post_marker(Leader& L, Group& G) {
  icpgpu_ctx* lead = G.lead;
  G.sync_seq = ++lead->post_seq;
  if (launch_post_ints(static_cast<const int*>(lead->batch_table.ptr), 1, lead->h_post_dev, wire_seq(lead, G.sync_seq), G.gstream) != hipSuccess) {
    fail(lead, ICPGPU_ERR_HIP, "lock-step batch: marker launch");
    return L.bail(ICPGPU_ERR_HIP, G.slots[0].pair, lead);
  }
  return 0;
}

// (2) the target grids, every build's host round trips shared by the group
int begin_builds(Leader& L, Group& G) {
  G.bt1 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < G.n_slots; ++i) {
    Slot& sl = G.slots[i];
    sl.gb = GridBuild{};
    if (sl.run.phase == P2PRun::Done) continue;  // empty target
    icpgpu_ctx* w = sl.w;
    const int mode = w->params.nn_mode;
    const bool want = mode == ICPGPU_NN_GRID || (mode == ICPGPU_NN_AUTO && w->tgt.n >= kGridMinTarget);
    const double cut = std::sqrt((double)sl.run.thr) * (1.0 + 1e-6);
    if (!want || !(sl.run.thr > 0.f) || !std::isfinite(cut) || cut > 1e6) {
      w->grid.usable = w->grid.built = false;
      continue;
    }
    const int rc = gb_begin(w, sl.gb, w->tgt, w->tgt_version, cut, /*adapt=*/true, w->grid);
    if (rc) return L.bail(rc, sl.pair, w);
  }
  if (post_marker(L, G)) return -1;
  G.phase = Group::Build;
  G.idle_spins = 0;
  return 1;
}

// (1) fill the group, ONE pair per step (a pair's host -> device copies occupy the thread for ~0.2 ms: the other
// groups' mailboxes are looked at in between)
int fill_step(Leader& L, Group& G) {
  BatchJob& job = L.job;
  if (G.n_slots == 0) {
    G.bt0 = std::chrono::steady_clock::now();
    // Ramp-up: groups that start together stay in phase -- all copying, then all building, then all sweeping, the chip idle
    // through the first two -- so the FIRST fill of the job's g-th group takes (g + 1) / n of a full group: the small ones
    // sweep (short steps, but on an otherwise idle chip) while the larger ones are still being copied in, and from then on
    // the groups finish and refill at different times.
    const size_t depth = job.plan.depth, total_groups = job.plan.n_threads * job.plan.groups_per_thread;
    G.cap = depth;
    if (!G.filled_once && stagger_on()) G.cap = std::max<size_t>(1, (depth * (G.index + 1) + total_groups - 1) / total_groups);
    G.filled_once = true;
  }
  size_t k = 0;
  if (G.n_slots != G.cap && job.claim(k)) {
    Slot& sl = G.slots[G.n_slots];
    sl.pair = k;
    sl.lock = sl.wants = sl.wants_fit = sl.waiting = false;
    int rc = job.load_pair(sl.w, k, /*sync=*/false);
    if (!rc) rc = p2p_prepare(sl.w, sl.run, nullptr, nullptr, job.want_fitness, &job.results[k]);
    if (rc) return L.bail(rc, k, sl.w);
    ++G.n_slots;
    if (G.n_slots < G.cap) return 1;
  }
  // full (or no pair left: the group goes with what it has)
  if (G.n_slots == 0 || job.abort.load()) {
    G.phase = Group::Retired;
    return 2;
  }
  return begin_builds(L, G);
}

// The stage's read-backs (hipMemcpyAsync into pinned memory, queued by the builds) have landed once the marker queued behind them
// has: polled in host memory, no runtime call and no sleeping wait; the stream is asked every 4096 empty looks.
// 1: landed, 0: not yet, < 0: failed.
int marker_landed(Leader& L, Group& G) {
  icpgpu_ctx* lead = G.lead;
  if ((lead->h_post[1] >> 24) < G.sync_seq) {
    if ((++G.idle_spins & 0xFFFu) != 0) return 0;
    const hipError_t q = hipStreamQuery(G.gstream);
    if (q != hipSuccess && q != hipErrorNotReady) {
      fail(G.slots[0].w, ICPGPU_ERR_HIP, "lock-step batch: %s", hipGetErrorString(q));
      return L.bail(ICPGPU_ERR_HIP, G.slots[0].pair, G.slots[0].w);
    }
    if (q == hipErrorNotReady) return 0;
    // (drained, with or without the marker -- its pair was torn or lost: the stream's word will do)
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  G.idle_spins = 0;
  return 1;
}

// a lock-step slot's row of the group's table: what nn_quad_batch_kernel and the batch reduction need of the pair
int table_entry(Leader& L, Group& G, size_t i) {
  Slot& sl = G.slots[i];
  icpgpu_ctx* w = sl.w;
  const int n_s = (int)w->src.n;
  const int flags = grid_flags(w->grid, false);
  if (w->src_grid.version != w->src_version) w->src_grid.built = w->src_grid.usable = false;
  const int blocks = grid_search_blocks(n_s);
  int rc = ensure(w, w->partials, (size_t)blocks * kReduceTerms * sizeof(double));
  bool use_prev = false;
  if (!rc) rc = prev_neighbours(w, w->grid, w->src.data(), n_s, flags, sl.prev, use_prev);  // (allocates; the first sweep is cold)
  if (rc) return L.bail(rc, sl.pair, w);
  w->prev.valid = w->tile_seed.valid = false;
  sl.pack = (flags & kGridPackShortRows) != 0;
  if (!rc) rc = ensure(w, w->keys, (size_t)n_s * sizeof(unsigned long long));
  if (!rc) rc = ensure(w, w->grid.unmatched, (size_t)(n_s + 1) * sizeof(int));
  if (rc) return L.bail(rc, sl.pair, w);
  BatchPair& bp = G.table[i];
  bp.keys = static_cast<unsigned long long*>(w->keys.ptr);
  bp.unmatched = static_cast<int*>(w->grid.unmatched.ptr);
  bp.unmatched_count = bp.unmatched + n_s;
  bp.r_max_open = std::min(4 * w->grid.g.r_max, 48);
  bp.src = w->src.data();
  bp.sorted = static_cast<const float4*>(w->grid.sorted.ptr);
  bp.cell_start = static_cast<const int*>(w->grid.cell_start.ptr);
  bp.partials = static_cast<double*>(w->partials.ptr);
  bp.prev_nn = sl.prev;
  bp.flags = w->h_flags_dev;
  bp.g = w->grid.g;
  bp.accept_thr = sl.run.thr;
  bp.n_s = n_s;
  bp.qpw = grid_search_qpw(n_s);
  bp.xcd_map = 0;
  bp.blocks = blocks;
  sl.wants = true;
  return 0;
}

// (3) who can iterate in lock-step; the others start their own first sweep
int open_iteration(Leader& L, Group& G) {
  icpgpu_ctx* lead = G.lead;
  G.bt2 = std::chrono::steady_clock::now();
  G.live = 0;
  for (size_t i = 0; i < G.n_slots; ++i) {
    Slot& sl = G.slots[i];
    if (sl.run.phase == P2PRun::Done) continue;
    icpgpu_ctx* w = sl.w;
    ++G.live;
    const int n_s = (int)w->src.n;
    sl.lock = grid_ready(w) && n_s > 0 && w->src.n < kOrderSourceMin && source_order_mode() != 1 &&
              grid_search_batchable(n_s, grid_flags(w->grid, false)) && sl.run.thr <= w->grid.cutoff * w->grid.cutoff;
    sl.run.phase = P2PRun::Iterating;
    sl.run.t_issue = std::chrono::steady_clock::now();
    if (!sl.lock) {
      int rc = ensure_source_order(w, sl.run.thr);
      if (!rc) rc = sweep_issue(w, to_xform(sl.run.final_T), sl.run.thr, false, sl.run.ticket);
      if (rc) return L.bail(rc, sl.pair, w);
      continue;
    }
    if (table_entry(L, G, i)) return -1;
  }
  // one row-walk variant for the whole group (the packed walk of sparse targets is a speed choice, the neighbours are the
  // same): the majority's, so that a step is ONE launch
  int n_lock = 0, n_pack = 0;
  for (size_t i = 0; i < G.n_slots; ++i)
    if (G.slots[i].lock) {
      ++n_lock;
      n_pack += G.slots[i].pack ? 1 : 0;
    }
  const bool group_pack = 2 * n_pack >= n_lock && n_pack > 0;
  for (size_t i = 0; i < G.n_slots; ++i) G.slots[i].pack = group_pack;
  if (hipMemcpyAsync(lead->batch_table.ptr, G.table.data(), G.n_slots * sizeof(BatchPair), hipMemcpyHostToDevice, G.gstream) != hipSuccess) {
    fail(lead, ICPGPU_ERR_HIP, "lock-step batch: table upload");
    return L.bail(ICPGPU_ERR_HIP, G.slots[0].pair, lead);
  }
  // the sweeps' stream takes over behind everything the builds' stream holds (the last build stage and the table are queued, not done)
  if (G.sstream != G.gstream &&
      (hipEventRecord(lead->ev[0], G.gstream) != hipSuccess || hipStreamWaitEvent(G.sstream, lead->ev[0], 0) != hipSuccess)) {
    fail(lead, ICPGPU_ERR_HIP, "lock-step batch: stream hand-over");
    return L.bail(ICPGPU_ERR_HIP, G.slots[0].pair, lead);
  }
  G.phase = Group::Iterate;
  G.idle_spins = 0;
  return 1;
}

// the builds' next stage once the last one's read-backs are there; when every grid stands, on to the iterations
int builds_step(Leader& L, Group& G) {
  bool pending = false;
  for (size_t i = 0; i < G.n_slots; ++i) pending = pending || G.slots[i].gb.state != GridBuild::Done;
  if (pending) {
    const int landed = marker_landed(L, G);
    if (landed <= 0) return landed;
    for (size_t i = 0; i < G.n_slots; ++i)
      if (G.slots[i].gb.state != GridBuild::Done) {
        const int rc = gb_advance(G.slots[i].w, G.slots[i].gb);
        if (rc) return L.bail(rc, G.slots[i].pair, G.slots[i].w);
      }
    pending = false;
    for (size_t i = 0; i < G.n_slots; ++i) pending = pending || G.slots[i].gb.state != GridBuild::Done;
    if (pending) {
      if (post_marker(L, G)) return -1;
      return 1;
    }
  }
  return open_iteration(L, G);
}

// kernel timing, sampled like the single-pair path's: a launch's HIP-event time / its pairs = one pair's sweep.  wait: the group
// closes and its last timed launch is finished, too; else only events that have already come are taken.
void take_timing(Group& G, bool wait) {
  icpgpu_ctx* lead = G.lead;
  if (!G.timed_pairs) return;
  if (!wait && hipEventQuery(lead->ev[3]) != hipSuccess) return;
  float ms = 0.f;
  if ((!wait || hipEventSynchronize(lead->ev[3]) == hipSuccess) && hipEventElapsedTime(&ms, lead->ev[2], lead->ev[3]) == hipSuccess) {
    lead->prof.grid_ms += (double)ms;  // (summed over the launch's pairs: grid_ms / grid_timed stays "per pair and sweep")
    lead->prof.grid_timed += (uint64_t)G.timed_pairs;
  }
  G.timed_pairs = 0;
}

// kind 1, per pair: the few points the grid left unmatched (completed on the device), then the keys-path reduction into
// the pair's mailbox -- three small launches each, queued without waiting
int fitness_tail(Leader& L, Group& G, const BatchStep& step, int n_act) {
  for (int a2 = 0; a2 < n_act; ++a2) {
    Slot& sl = G.slots[step.slot[a2]];
    icpgpu_ctx* w = sl.w;
    const BatchPair& bp = G.table[step.slot[a2]];
    hipError_t e2 = launch_nn_brute_few(w->src.data(), bp.unmatched, bp.unmatched_count, 0, w->tgt.data(), (int)w->tgt.n,
                                        step.T[a2], bp.keys, reinterpret_cast<int*>(w->h_sums_dev + 20), G.sstream);
    int rc2 = e2 == hipSuccess ? ensure(w, w->partials, (size_t)kMaxReduceBlocks * kReduceTerms * sizeof(double)) : ICPGPU_ERR_HIP;
    if (!rc2 && launch_reduce(w->src.data(), (int)w->src.n, w->tgt.data(), bp.keys, step.T[a2], FLT_MAX,
                              static_cast<double*>(w->partials.ptr), w->h_sums_dev, w->h_flags_dev, step.seq[a2], G.sstream) != hipSuccess)
      rc2 = ICPGPU_ERR_HIP;
    if (rc2) {
      fail(w, rc2, "lock-step batch: fitness sweep");
      return L.bail(rc2, sl.pair, w);
    }
  }
  return 0;
}

// (4) one step of one kind (0: the gated sweeps due, 1: the fitness sweeps due): one search launch + one reduction launch for
// every pair of the group that wants it
int launch_step(Leader& L, Group& G, int kind) {
  icpgpu_ctx* lead = G.lead;
  BatchStep step;
  int n_act = 0, max_blocks = 0;
  bool group_pack = false;
  step.use_prev_mask = 0u;
  for (size_t i = 0; i < G.n_slots; ++i) {
    Slot& sl = G.slots[i];
    if (!sl.lock || !(kind == 0 ? sl.wants : sl.wants_fit)) continue;
    icpgpu_ctx* w = sl.w;
    const BatchPair& bp = G.table[i];
    group_pack = sl.pack;
    bool use_prev = false;
    unsigned int* buf = nullptr;
    if (prev_neighbours(w, w->grid, w->src.data(), (int)w->src.n, grid_flags(w->grid, false), buf, use_prev) || buf != sl.prev) {
      fail(w, ICPGPU_ERR_HIP, "lock-step batch: previous-neighbour buffer moved");
      return L.bail(ICPGPU_ERR_HIP, sl.pair, w);
    }
    step.T[n_act] = to_xform(sl.run.final_T);
    step.seq[n_act] = wire_seq(w, ++w->sums_seq);
    step.slot[n_act] = (unsigned char)i;
    if (use_prev) step.use_prev_mask |= 1u << n_act;
    max_blocks = std::max(max_blocks, bp.blocks);
    sl.run.ticket = SweepTicket{};
    sl.run.ticket.seq = w->sums_seq;
    sl.run.t_issue = std::chrono::steady_clock::now();
    sl.wants = sl.wants_fit = false;
    sl.waiting = true;
    w->call_sweeps += 1;
    w->prof.grid_launches += 1;
    w->prof.reduce_launches += 1;
    w->prof.grid_bytes += 16ull * ((uint64_t)w->src.n + (uint64_t)w->tgt.n) +
                          (kind == 0 ? 136ull * (uint64_t)bp.blocks : 8ull * (uint64_t)w->src.n);
    w->prof.reduce_bytes += kind == 0 ? 136ull * (uint64_t)bp.blocks : 40ull * (uint64_t)w->src.n + 136;
    if (kind == 1) {  // the ungated sweep's set-up, as sweep_issue / nn_keys_grid do it for one pair
      sl.run.ticket.few_host = reinterpret_cast<volatile int*>(w->h_sums + 20);
      *sl.run.ticket.few_host = -1;
      sl.run.ticket.red_src = w->src.data();
      sl.run.ticket.red_n = (int)w->src.n;
      sl.run.ticket.T = step.T[n_act];
      sl.run.ticket.thr = FLT_MAX;
      if (hipMemsetAsync(bp.unmatched_count, 0, sizeof(int), G.sstream) != hipSuccess) {
        fail(w, ICPGPU_ERR_HIP, "lock-step batch: memset");
        return L.bail(ICPGPU_ERR_HIP, sl.pair, w);
      }
    }
    ++n_act;
  }
  if (n_act == 0) return 0;
  L.bt_steps += 1;
  take_timing(G, /*wait=*/false);
  const bool timed = kind == 0 && G.timed_pairs == 0 && (G.step_counter++ % 5u) == 0;
  if (timed) (void)hipEventRecord(lead->ev[2], G.sstream);
  const BatchPair* d_table = static_cast<const BatchPair*>(lead->batch_table.ptr);
  hipError_t e = launch_nn_grid_search_batch(d_table, step, n_act, max_blocks, group_pack, kind == 1, G.sstream);
  if (timed) {
    (void)hipEventRecord(lead->ev[3], G.sstream);
    G.timed_pairs = n_act;
  }
  if (e == hipSuccess && kind == 0) e = launch_reduce_final_batch(d_table, step, n_act, G.sstream);
  if (e != hipSuccess) {
    fail(lead, ICPGPU_ERR_HIP, "lock-step batch launch: %s", hipGetErrorString(e));
    return L.bail(ICPGPU_ERR_HIP, G.slots[step.slot[0]].pair, lead);
  }
  return kind == 1 ? fitness_tail(L, G, step, n_act) : 0;
}

// take everything that has come back: the host's share of an iteration for every pair whose sums are there
int collect(Leader& L, Group& G, bool& progressed) {
  progressed = false;
  for (size_t i = 0; i < G.n_slots; ++i) {
    Slot& sl = G.slots[i];
    if (!sl.awaited()) continue;
    if (sl.lock && !sl.waiting) continue;  // its sweep has not been launched yet
    if (!sweep_ready(sl.w, sl.run.ticket)) continue;
    sl.waiting = false;
    int deferred = 0;
    const int rc = p2p_advance(sl.w, sl.run, (sl.lock && sl.run.phase == P2PRun::Iterating) ? &deferred : nullptr);
    if (rc) return L.bail(rc, sl.pair, sl.w);
    sl.wants = deferred == 1;
    sl.wants_fit = deferred == 2;
    if (sl.run.phase == P2PRun::Done) --G.live;
    progressed = true;
  }
  return 0;
}

// nothing moved for a while: the group's streams are asked once, the verdict and the clock go to every pair that is awaited
int stalled(Leader& L, Group& G) {
  bool asked = false;
  for (size_t i = 0; i < G.n_slots; ++i) {
    Slot& sl = G.slots[i];
    if (!sl.awaited()) continue;
    const int rc = asked ? batch_stall_look(sl.w, {}, sl.run.t_issue) : batch_stall_look(sl.w, {G.sstream, G.gstream}, sl.run.t_issue);
    if (rc) return L.bail(ICPGPU_ERR_HIP, sl.pair, sl.w);
    asked = true;
  }
  return 0;
}

// the group is finished: its last timed launch, the development flavour's traces, and back to filling
int close_group(Leader& L, Group& G) {
  take_timing(G, /*wait=*/true);
  if (bt_trace()) {  // development flavour, ICPGPU_BATCH_TRACE=1: the round's phase boundaries, ms after the call started
    const auto ms = [&](std::chrono::steady_clock::time_point tp) { return std::chrono::duration<double, std::milli>(tp - L.job.t_call).count(); };
    fprintf(stderr, "[icpgpu] batch trace: thread %zu group %zu: %zu pairs | fill %.2f .. %.2f | builds .. %.2f | sweeps .. %.2f\n", L.t, G.index, G.n_slots,
            ms(G.bt0), ms(G.bt1), ms(G.bt2), ms(std::chrono::steady_clock::now()));
  }
  if (bt_on()) {
    const auto bt3 = std::chrono::steady_clock::now();
    L.bt_fill += std::chrono::duration<double, std::milli>(G.bt1 - G.bt0).count();
    L.bt_build += std::chrono::duration<double, std::milli>(G.bt2 - G.bt1).count();
    L.bt_iter += std::chrono::duration<double, std::milli>(bt3 - G.bt2).count();
    L.bt_groups += 1;
  }
  G.n_slots = 0;
  G.phase = Group::Fill;
  return 1;
}

// (4) iterate: one search launch + one reduction launch per step and row-walk class for the whole group
int iterate_step(Leader& L, Group& G) {
  if (G.live == 0) return close_group(L, G);
  // a step is launched when no lock-step sweep of the group is in flight any more (the step IS the batch; pairs in
  // their fitness sweep or on the single-pair path do not hold it up)
  bool lock_in_flight = false;
  for (size_t i = 0; i < G.n_slots; ++i) lock_in_flight = lock_in_flight || (G.slots[i].lock && G.slots[i].waiting);
  for (int kind = 0; kind < 2 && !lock_in_flight; ++kind)
    if (launch_step(L, G, kind)) return -1;
  bool progressed = false;
  if (collect(L, G, progressed)) return -1;
  if (!progressed) {
    if ((++G.idle_spins & 0x3FFu) == 0 && stalled(L, G)) return -1;
    return 0;
  }
  G.idle_spins = 0;
  return G.live > 0 ? 1 : close_group(L, G);
}

// One non-blocking step of a group.  1: something moved, 0: nothing did, 2: the group is retired (no pairs left), < 0: failed
// (the thread's error is set).
int group_step(Leader& L, Group& G) {
  switch (G.phase) {
    case Group::Fill: return fill_step(L, G);
    case Group::Build: return builds_step(L, G);
    case Group::Iterate: return iterate_step(L, G);
    default: return 2;
  }
}

}  // namespace

void run_lockstep_groups(BatchJob& job, size_t t) {
  icpgpu_ctx* c = job.c;
  const size_t depth = job.plan.depth, n_threads = job.plan.n_threads;
  icpgpu_ctx* const* ws = job.workers_of(t);
  Leader L{job, t};
  std::vector<Group> groups(job.plan.groups_per_thread);
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    Group& G = groups[gi];
    G.ws = ws + gi * depth;
    G.index = gi * n_threads + t;  // (a thread's groups are far apart: its first one starts early, its last one late)
    G.lead = G.ws[0];
    // The group's stream is one of those the call created in a row (icpgpu_batch.cpp: spread over the hardware queues in creation order)
    G.gstream = c->group_streams[G.index];
    // (Measured and dropped in round 5: the sweeps on a stream of the LOWEST priority, so that the small kernels of another group's
    // index build -- 1-5 ms per group on a busy chip, 0.4 ms on an idle one -- are dispatched ahead of the waiting sweep
    // workgroups: 15-25 % SLOWER in every configuration, copies stalling for milliseconds; profiles/r05_batch_groups.txt.)
    G.sstream = G.gstream;
    G.slots.resize(depth);
    G.table.resize(depth);
    G.own.resize(depth);
    for (size_t s2 = 0; s2 < depth; ++s2) {
      G.slots[s2].w = G.ws[s2];
      G.own[s2] = G.ws[s2]->stream;
      G.ws[s2]->stream = G.gstream;  // one queue for the group: builds, sweeps and fitness sweeps are ordered by it
    }
    if (ensure(G.lead, G.lead->batch_table, depth * sizeof(BatchPair))) return job.failed(t, ICPGPU_ERR_OOM, 0, G.lead);
  }
  // ONE group of the thread fills at a time (the others wait their turn): its pairs are complete and iterating while the next
  // group's are still being copied in, so the thread's groups run staggered -- copies under sweeps -- instead of in phase
  size_t fill_owner = 0;
  for (size_t retired = 0; retired < groups.size();) {
    bool moved = false;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      Group& G = groups[gi];
      if (G.phase == Group::Retired) continue;
      if (G.phase == Group::Fill && gi != fill_owner) {
        if (groups[fill_owner].phase == Group::Fill) continue;
        fill_owner = gi;
      }
      const int r = group_step(L, G);
      if (r < 0) return;
      if (r == 2) ++retired;
      moved = moved || r != 0;
    }
#if defined(__x86_64__)
    if (!moved) __builtin_ia32_pause();
#endif
  }
}

}  // namespace icpgpu_impl
