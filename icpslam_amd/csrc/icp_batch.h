// icp_batch.h -- what the host threads of one icpgpu_align_batch call share (INTERNAL; icpgpu_batch.cpp, icpgpu_batch_lockstep.cpp).
#pragma once
#include "icp_ctx.h"
#include "icp_batch_plan.h"

#pragma GCC visibility push(hidden)  // shared by two units of the library, exported by neither
namespace icpgpu_impl {

struct ThreadError {  // one slot per host thread: nothing shared is written while the threads run
  int code = ICPGPU_OK;
  size_t pair = 0;
  std::string msg;
};

struct BatchJob {
  icpgpu_ctx* c = nullptr;
  size_t n_pairs = 0;
  const float* const* src = nullptr;
  const size_t* n_src = nullptr;
  const float* const* tgt = nullptr;
  const size_t* n_tgt = nullptr;
  int want_fitness = 0;
  icpgpu_result* results = nullptr;
  BatchPlan plan;
  std::atomic<size_t> next{0};
  std::atomic<bool> abort{false};
  std::chrono::steady_clock::time_point t_call;
  std::vector<ThreadError> errors;

  icpgpu_ctx* const* workers_of(size_t t) const { return &c->workers[t * plan.per_thread()]; }
  int load_pair(icpgpu_ctx* w, size_t k, bool sync = true) const {  // (the caller's buffers outlive this call: sync is optional)
    w->src_version++;
    int rc = set_cloud_host(w, w->src, src[k], n_src[k], sync);
    w->tgt_version++;
    if (!rc) rc = set_cloud_host(w, w->tgt, tgt[k], n_tgt[k], sync);
    return rc;
  }
  // the pairs are dealt dynamically: false when none is left or a thread has failed
  bool exhausted() const { return next.load() >= n_pairs; }
  bool claim(size_t& k) {
    if (abort.load() || exhausted()) return false;
    k = next.fetch_add(1);
    return k < n_pairs;
  }
  void failed(size_t t, int rc, size_t k, icpgpu_ctx* w) {
    errors[t].code = rc;
    errors[t].pair = k;
    errors[t].msg = w->err;
    abort.store(true);
  }
};

// One look of the schedulers' watchdog at a run whose result has not come for a while (the callers look once per 1024 idle spins): a
// faulted or hung kernel must not keep a thread spinning.  The streams in `ask` are asked first; one that has drained is no error
// (the result is on its way through host memory, or the run waits for another stream): the run keeps waiting, the clock still runs.
// 0: wait on, < 0: reported on w.
inline int batch_stall_look(icpgpu_ctx* w, std::initializer_list<hipStream_t> ask, std::chrono::steady_clock::time_point t_issue) {
  const WaitNames names{"a reduction", "a kernel's result"};
  for (hipStream_t st : ask) {
    const int asked = wait_ask_stream(w, st, names);  // (WhenIdle::KeepWaiting in icp_wait.h's terms)
    if (asked < 0) return asked;
  }
  if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_issue).count() > wait_timeout_ms()) return wait_timed_out(w, names);
  return 0;
}

// a host thread's lock-step groups, start to finish (icpgpu_batch_lockstep.cpp)
void run_lockstep_groups(BatchJob& job, size_t t);

}  // namespace icpgpu_impl
#pragma GCC visibility pop
