// icp_wait.h -- the library's one wait for a result that a kernel posts into host-visible memory (included by icp_ctx.h).
// The host looks at the mailbox; every 1024 looks it asks the stream, so that a faulted kernel becomes an error, and the clock, so
// that a hung one does (wait_timeout_ms).  Two forms: wait_mailbox spins until the result is there, poll_mailbox is one look of a
// resumable run that has just found its mailbox empty.  What a caller does about a stream that has DRAINED without the result
// differs from caller to caller, on purpose: both forms hand that case back (1) and every call site says what it makes of it.
#pragma once

namespace icpgpu_impl {

// what the messages call the thing waited for: "HIP error while waiting for <what>: ..." and "timed out after ... waiting for
// <late> (hung kernel?)" -- the reductions' two messages name it differently
struct WaitNames {
  const char* what;
  const char* late;
  WaitNames(const char* w) : what(w), late(w) {}
  WaitNames(const char* w, const char* l) : what(w), late(l) {}
};
enum class WhenIdle { Report, KeepWaiting };  // a drained stream: hand it to the caller, or wait on (the clock still runs)

// one question to the stream: 0 = still working, 1 = drained, < 0 = a HIP error (reported)
inline int wait_ask_stream(icpgpu_ctx* c, hipStream_t stream, const WaitNames& names) {
  const hipError_t q = hipStreamQuery(stream);
  if (q == hipSuccess) return 1;
  if (q == hipErrorNotReady) return 0;
  return fail(c, ICPGPU_ERR_HIP, "HIP error while waiting for %s: %s", names.what, hipGetErrorString(q));
}
inline int wait_timed_out(icpgpu_ctx* c, const WaitNames& names) {
  return fail(c, ICPGPU_ERR_HIP, "timed out after %.0f ms waiting for %s (hung kernel?)", wait_timeout_ms(), names.late);
}

// Blocking: 0 = ready() said yes (acquire fence taken), 1 = the stream drained and ready() still says no, < 0 = error.  The clock
// starts with the first question to the stream.  yield_after: spins after which the loop yields the core instead of pausing (0: never).
template <class Ready>
inline int wait_mailbox(icpgpu_ctx* c, hipStream_t stream, const WaitNames& names, Ready&& ready, WhenIdle idle = WhenIdle::Report,
                        unsigned yield_after = 0) {
  std::chrono::steady_clock::time_point t0;
  for (unsigned spins = 1;; ++spins) {
    if (ready()) break;
    if ((spins & 0x3FFu) == 0) {
      const int asked = wait_ask_stream(c, stream, names);
      if (asked < 0) return asked;
      if (asked == 1 && idle == WhenIdle::Report) {  // everything retired: the result must be there on the next look
        if (ready()) break;
        return 1;
      }
      const auto now = std::chrono::steady_clock::now();
      if (spins == 0x400u) t0 = now;
      else if (std::chrono::duration<double, std::milli>(now - t0).count() > wait_timeout_ms()) return wait_timed_out(c, names);
    }
    if (yield_after && spins > yield_after) std::this_thread::yield();
#if defined(__x86_64__)
    else __builtin_ia32_pause();
#endif
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

// Polling: the caller has looked and found nothing.  0 = not yet, 1 = the stream has drained (look once more: what is not there
// now will not come), < 0 = error.  polls: the run's count of empty looks; t_issue: when the awaited work was queued.
inline int poll_mailbox(icpgpu_ctx* c, hipStream_t stream, const WaitNames& names, unsigned& polls,
                        std::chrono::steady_clock::time_point t_issue, WhenIdle idle = WhenIdle::Report) {
  if ((++polls & 0x3FFu) != 0) return 0;
  const int asked = wait_ask_stream(c, stream, names);
  if (asked < 0) return asked;
  if (asked == 1 && idle == WhenIdle::Report) return 1;
  if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_issue).count() > wait_timeout_ms()) return wait_timed_out(c, names);
  return 0;
}

}  // namespace icpgpu_impl
