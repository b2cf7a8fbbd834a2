// The streams of the native runtime beside the caller's (misa_handle.h: SideStream, BgStream): fork, join and flag join with the
// side stream, the background stream of the embedding table's pass, the device copy of the run table, the timing events -- and
// where each of those resources is created and released.  The only misa*.hip file with device code: the two flag kernels.
#include "misa_handle.h"

using namespace mmda_step;
using namespace misa_rt;

namespace {
unsigned fork_event_flags() {
  static const int sysfence = mmda_env_int("MMDA_EVENT_SYSFENCE", 0);
  return hipEventDisableTiming | (sysfence ? 0u : hipEventDisableSystemFence);
}
__global__ void flag_wait_kernel(const unsigned* flag, unsigned value, unsigned* err) { flag_wait(flag, value, err); }
__global__ void flag_set_kernel(unsigned* flag, unsigned value) {
  __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
}  // namespace

namespace misa_rt {

void ev_rec(mmda_misa* m, int step, int slot, int which, void* stream) {
  if (m->tm.ev.empty() || step >= m->tm.ev_steps) return;
  if ((slot < 2 ? m->tm.ev_seen_f : m->tm.ev_seen_b) % m->set.ev_stride) return;
  if (m->set.ev_rotate && slot != (step & 3)) return;
  (void)hipEventRecord(m->tm.ev[(step * 4 + slot) * 2 + which], (hipStream_t)stream);
  if (which == 1 && (size_t)(step * 4 + slot) < m->tm.ev_done.size()) m->tm.ev_done[step * 4 + slot] = 1;
}

// Fork: work issued on the returned stream starts after everything already on `main_stream` and runs beside what follows
// there; side_join() makes `main_stream` wait for it.  Without overlap the main stream itself is returned.
int side_fork(mmda_misa* m, void* main_stream, void** out) {
  *out = main_stream;
  if (!m->set.use_side) return MMDA_OK;
  if (!m->sd.side) { const int rc = m->sd.create(fork_event_flags()); if (rc) return rc; }
  if (hipEventRecord(m->sd.ev_fork, (hipStream_t)main_stream) != hipSuccess) return MMDA_ELAUNCH;
  if (hipStreamWaitEvent(m->sd.side, m->sd.ev_fork, 0) != hipSuccess) return MMDA_ELAUNCH;
  m->sd.side_pending = 1;
  *out = m->sd.side;
  return MMDA_OK;
}
int side_launch(mmda_misa* m, std::vector<mmda_gemm_args>& list, void* main_stream) {
  if (list.empty()) return MMDA_OK;
  void* ss = nullptr;
  int rc = side_fork(m, main_stream, &ss);
  if (!rc) rc = mmda_gemm_grouped(list.data(), (int)list.size(), ss);
  list.clear();
  return rc;
}
// the side stream's chain ends here for the main stream: word `idx` is set behind it (flag join) -- or was, by the chain's last launch
// itself (by_kernel) --; ev_join is recorded too
int side_flag_signal(mmda_misa* m, int idx, bool by_kernel) {
  if (!m->sd.side || !m->sd.jflags) return MMDA_EINVAL;
  ++m->sd.jval[idx];
  if (!by_kernel) {
    hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(1), 0, m->sd.side, m->sd.jflags + idx, m->sd.jval[idx]);
    MMDA_CHECK_LAUNCH("side_flag_signal");
  }
  if (hipEventRecord(m->sd.ev_join, m->sd.side) != hipSuccess) return MMDA_ELAUNCH;
  m->sd.side_pending = 0;
  return MMDA_OK;
}
// a flag join whose consumer kernel will not run after all: the event recorded with it
int flag_join_fallback(mmda_misa* m, void* main_stream) {
  if (hipStreamWaitEvent((hipStream_t)main_stream, m->sd.ev_join, 0) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}
int side_join(mmda_misa* m, void* main_stream) {
  if (!m->sd.side_pending) return MMDA_OK;
  if (hipEventRecord(m->sd.ev_join, m->sd.side) != hipSuccess) return MMDA_ELAUNCH;
  if (hipStreamWaitEvent((hipStream_t)main_stream, m->sd.ev_join, 0) != hipSuccess) return MMDA_ELAUNCH;
  m->sd.side_pending = 0;
  return MMDA_OK;
}
// the sorted id list's word, [3]: set behind the sort on the side stream, waited for by one wave on the main stream
int esort_signal(mmda_misa* m, void* side_stream) {
  hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)side_stream, m->sd.jflags + 3, ++m->sd.esort_val);
  return hipGetLastError() != hipSuccess ? MMDA_ELAUNCH : MMDA_OK;
}
int esort_wait(mmda_misa* m, void* main_stream) {
  hipLaunchKernelGGL(flag_wait_kernel, dim3(1), dim3(64), 0, (hipStream_t)main_stream, m->sd.jflags + 3, m->sd.esort_val, m->sd.jflags + 2);
  return hipGetLastError() != hipSuccess ? MMDA_ELAUNCH : MMDA_OK;
}

// ---- the background pass over the embedding table (see BgStream)
// Its stream, events and stamps, made once; then the step's epoch.  What the launch that reads the n ids stamps with: *st.
int bg_begin(mmda_misa* m, const int64_t* ids, int n, void* main_stream, RowStamp* st) {
  const size_t bytes = sizeof(unsigned) * (size_t)m->cfg.vocab;
  { const int rc = m->bgp.create(bytes, fork_event_flags()); if (rc) return rc; }
  if (!m->bgp.ev_bg_fork || !m->bgp.ev_bg_done) return MMDA_ELAUNCH;
  if (++m->bgp.bg_epoch == 0u) {                             // wrapped: a stamp of 2^32 steps ago would read as this step's
    if (hipMemsetAsync(m->bgp.row_stamp, 0, bytes, (hipStream_t)main_stream) != hipSuccess) return MMDA_ELAUNCH;
    m->bgp.bg_epoch = 1u;
  }
  *st = RowStamp{m->bgp.row_stamp, m->bgp.bg_epoch, m->cfg.vocab, ids, n};
  return MMDA_OK;
}
// the fork and the pass (the step's optimizer step: `opt`): behind everything `main_stream` holds
int bg_launch(mmda_misa* m, const OptStep* opt, void* main_stream) {
  if (!opt || !m->bgp.bg || !m->bgp.row_stamp) return MMDA_EINVAL;
  if (hipEventRecord(m->bgp.ev_bg_fork, (hipStream_t)main_stream) != hipSuccess) return MMDA_ELAUNCH;
  if (hipStreamWaitEvent(m->bgp.bg, m->bgp.ev_bg_fork, 0) != hipSuccess) return MMDA_ELAUNCH;
  const int64_t e = m->par.embed;
  const int rc = mmda_adam_background_launch(m->P + e, m->M1 + e, m->V1 + e, bg_table(m), bg_hyper(m, *opt), m->st.plan.embed_bg_wgs,
                                             m->st.plan.embed_bg_lds, m->bgp.bg);
  if (rc) return rc;
  m->bgp.bg_pending = 1; m->bgp.bg_active = 1;                   // (from here on rows may have taken the step, whatever the step returns)
  if (hipEventRecord(m->bgp.ev_bg_done, m->bgp.bg) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}
// join: `stream` (the side stream in front of its flag word, or the main stream) goes on only when the pass is through
int bg_join(mmda_misa* m, void* stream) {
  if (!m->bgp.bg_pending) return MMDA_OK;
  if (hipStreamWaitEvent((hipStream_t)stream, m->bgp.ev_bg_done, 0) != hipSuccess) return MMDA_ELAUNCH;
  m->bgp.bg_pending = 0;
  return MMDA_OK;
}

// the table on the device, current.  A changed set waits for the streams that may still read the old table: once per change.
int runs_ready(mmda_misa* m, void* stream) {
  if (!m->rd.runs_dirty && m->rd.runs_dev) return MMDA_OK;
  const int need = (int)m->set.runs.size();
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return MMDA_ELAUNCH;
  if (m->sd.side && hipStreamSynchronize(m->sd.side) != hipSuccess) return MMDA_ELAUNCH;
  if (need > m->rd.runs_dev_cap) {
    if (m->rd.runs_dev) (void)hipFree(m->rd.runs_dev);
    m->rd.runs_dev = nullptr; m->rd.runs_dev_cap = 0;
    const int cap = (int)m->par.params.size() + 1;            // every tensor a run of its own, and the closing entry
    if (hipMalloc(reinterpret_cast<void**>(&m->rd.runs_dev), sizeof(mmda_run) * cap) != hipSuccess) { m->rd.runs_dev = nullptr; return MMDA_ELAUNCH; }
    m->rd.runs_dev_cap = cap;
  }
  if (hipMemcpy(m->rd.runs_dev, m->set.runs.data(), sizeof(mmda_run) * need, hipMemcpyHostToDevice) != hipSuccess) return MMDA_ELAUNCH;
  m->rd.runs_dirty = 0;
  return MMDA_OK;
}

// ---- the resources' create / release (the types: misa_handle.h)
int SideStream::create(unsigned evf) {
  if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) return MMDA_ELAUNCH;
  // The fork / join events order streams of ONE device: no system-scope fence with them (hipEventDisableSystemFence -- "device
  // memory may not be visible to the host and other devices", neither of which waits on these events; every kernel still ends with
  // its own device-scope release).  With the fence a recorded event costs the recording stream 6 us between two launches, without
  // it 3 (tools/micro/fork_cost.hip).  MMDA_EVENT_SYSFENCE=1: with the fence.
  if (hipEventCreateWithFlags(&ev_fork, evf) != hipSuccess) return MMDA_ELAUNCH;
  if (hipEventCreateWithFlags(&ev_join, evf) != hipSuccess) return MMDA_ELAUNCH;
  if (hipEventCreateWithFlags(&ev_pack, evf) != hipSuccess) return MMDA_ELAUNCH;
  if (hipMalloc(reinterpret_cast<void**>(&jflags), 64) != hipSuccess) { jflags = nullptr; return MMDA_ELAUNCH; }
  if (hipMemset(jflags, 0, 64) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}
void SideStream::release_events() {
  if (ev_fork) (void)hipEventDestroy(ev_fork);
  if (ev_join) (void)hipEventDestroy(ev_join);
  if (ev_pack) (void)hipEventDestroy(ev_pack);
  if (ev_early) (void)hipEventDestroy(ev_early);
}
void SideStream::release() {
  if (side) (void)hipStreamDestroy(side);
  if (jflags) (void)hipFree(jflags);
}
int BgStream::create(size_t bytes, unsigned evf) {
  if (!bg) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return MMDA_ELAUNCH;
    if (hipStreamCreateWithPriority(&bg, hipStreamNonBlocking, least) != hipSuccess) { bg = nullptr; return MMDA_ELAUNCH; }
    if (hipEventCreateWithFlags(&ev_bg_fork, evf) != hipSuccess) return MMDA_ELAUNCH;
    if (hipEventCreateWithFlags(&ev_bg_done, evf) != hipSuccess) return MMDA_ELAUNCH;
  }
  if (!row_stamp) {
    if (hipMalloc(reinterpret_cast<void**>(&row_stamp), bytes) != hipSuccess) { row_stamp = nullptr; return MMDA_ELAUNCH; }
    if (hipMemset(row_stamp, 0, bytes) != hipSuccess) return MMDA_ELAUNCH;
    bg_epoch = 0u;
  }
  return MMDA_OK;
}
void BgStream::release() {
  if (bg) { (void)hipStreamSynchronize(bg); (void)hipStreamDestroy(bg); }
  if (ev_bg_fork) (void)hipEventDestroy(ev_bg_fork);
  if (ev_bg_done) (void)hipEventDestroy(ev_bg_done);
  if (row_stamp) (void)hipFree(row_stamp);
}
void RunsDev::release() {
  if (runs_dev) (void)hipFree(runs_dev);
}
void Timing::release() {
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
}

}  // namespace misa_rt

extern "C" int mmda_misa_timing_end(mmda_misa* m) {
  if (!m) return MMDA_EINVAL;
  m->tm.release();
  m->tm.ev.clear(); m->tm.ev_steps = m->tm.ev_fwd = m->tm.ev_bwd = 0; m->tm.ev_seen_f = m->tm.ev_seen_b = 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_timing_stride(mmda_misa* m, int stride) {
  if (!m || stride < 1) return MMDA_EINVAL;
  m->set_mut().ev_stride = stride;
  return MMDA_OK;
}
extern "C" int mmda_misa_timing_begin(mmda_misa* m, int max_steps) {
  if (!m || max_steps <= 0 || max_steps > 4096) return MMDA_EINVAL;
  mmda_misa_timing_end(m);
  m->tm.ev.resize((size_t)max_steps * 8);
  // (timing events only: without the system-scope fence -- cache write-back and invalidation -- a default event performs when it is
  //  recorded, which is what hipEventDisableSystemFence is for: a sampled step costs the run half as much)
  for (auto& e : m->tm.ev)
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return MMDA_ELAUNCH;
  m->tm.ev_steps = max_steps;
  m->tm.ev_done.assign((size_t)max_steps * 4, 0);
  return MMDA_OK;
}
extern "C" int mmda_misa_timing_rotate(mmda_misa* m, int on) {
  if (!m) return MMDA_EINVAL;
  m->set_mut().ev_rotate = on ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_timing_collect(mmda_misa* m, float mean_ms[4], int* steps) {
  if (!m || !mean_ms || m->tm.ev.empty()) return MMDA_EINVAL;
  int n = m->tm.ev_fwd < m->tm.ev_bwd ? m->tm.ev_fwd : m->tm.ev_bwd;
  if (n > m->tm.ev_steps) n = m->tm.ev_steps;
  double acc[4] = {0, 0, 0, 0};
  int cnt[4] = {0, 0, 0, 0};
  for (int s = 0; s < n; ++s)
    for (int k = 0; k < 4; ++k) {
      if ((size_t)(s * 4 + k) >= m->tm.ev_done.size() || !m->tm.ev_done[s * 4 + k]) continue;      // (rotation: one launch per sampled step)
      float ms = 0.f;
      if (hipEventSynchronize(m->tm.ev[(s * 4 + k) * 2 + 1]) != hipSuccess) return MMDA_ELAUNCH;
      if (hipEventElapsedTime(&ms, m->tm.ev[(s * 4 + k) * 2], m->tm.ev[(s * 4 + k) * 2 + 1]) != hipSuccess) return MMDA_ELAUNCH;
      acc[k] += ms; cnt[k]++;
    }
  int least = n;
  for (int k = 0; k < 4; ++k) { mean_ms[k] = cnt[k] > 0 ? (float)(acc[k] / cnt[k]) : 0.f; least = cnt[k] < least ? cnt[k] : least; }
  if (steps) *steps = least;                            // samples behind every mean (the least-sampled launch)
  return MMDA_OK;
}
