// Native runtime for one MISA training iteration (reference loop body solver.py:139-186 over models.py:163-285).
// Host-side C++ only: holds the parameter table, the workspace carve and the step's plan (step_plan.h makes all three), and issues the
// HIP kernels of gemm.hip / lstm.hip / norm.hip / embed_rows.hip / attn.hip / losses.hip / optim.hip in dependency order on one
// stream.  No device memory is owned here; no torch types; no host<->device synchronisation anywhere in a step.
#include "step_plan.h"
#include <algorithm>
#include <cstring>

using namespace mmda_step;

namespace {

enum { SITE_ATTN = 1, SITE_DROP1 = 2, SITE_FFN = 3, SITE_DROP2 = 4, SITE_CLS = 5, SITE_DISC = 6,
       SITE_RRELU = 7 /* .. 9: the three projections' random slopes */, SITE_RRELU_DISC = 10 };

// The scalars of one optimizer step.  acc: an accumulator added to the gradient, or nullptr; norm: clip_grad_norm_ in front of it.
struct OptStep { float lr, clip, grad_scale; int step; const float* acc; bool norm; };
// The id list and lengths of a backward whose rows update is still to run (the caller keeps them alive, as it does for backward itself)
struct PendingRows {
  const int64_t* ids = nullptr; const int32_t* lengths = nullptr; bool on = false;
  void set(const int64_t* i, const int32_t* l) { ids = i; lengths = l; on = true; }
  PendingRows take() { const PendingRows r = *this; *this = PendingRows{}; return r; }
};
struct RowList { int64_t* ids; float* rows; int64_t used, capacity; };   // an accumulated step's (ids, rows) list: sparse table
// What one forward pass is asked to be: the parameters of that call, handed down to it (the handle keeps settings and outcomes)
struct StepRequest {
  bool fused = false;            // called from train_step: eager side losses, flag joins, the bucket clear rides inside forward
  const float* emo = nullptr;    // labels of a fused step (loss seeds stored by the forward stretches)
  const OptStep* opt = nullptr;  // the optimizer step behind this pass, where its kind may start early work (background table pass)
  bool enc_cached = false;       // the forward starts behind the encoders
};

}  // namespace

struct mmda_misa {
  explicit mmda_misa(const mmda_misa_config& c) : cfg(c), par(build_params(c)) {}
  mmda_misa(const mmda_misa&) = delete;      // (`lay` refers to this handle's own value)
  mmda_misa_config cfg;                      // fixed at create, but for cfg.mode (mmda_misa_set_mode)
  const ParamTable par;                      // fixed at create
  const Workspace& lay = lay_;               // the carve of the bound (B, T): read-only but for ...
  void rebind(const Workspace& v) { lay_ = v; }   // ... mmda_misa_set_workspace_async, which replaces it as a whole
  // ---- bound buffers (mmda_misa_bind, mmda_misa_set_workspace_async)
  float *P = nullptr, *G = nullptr, *M1 = nullptr, *V1 = nullptr;
  float* ws = nullptr;
  // cluster-exchange regions: at the front of the workspace, sized by B alone, so a change of T (every batch under the reference's
  // collate) neither moves nor clears them -- flags are monotonic epochs.  Cleared (on the caller's stream) only when the buffer
  // or B changes; the abort words found there before a clear are kept in `abort_sticky`.
  float* xchg_ws = nullptr; int xchg_B = 0; int abort_sticky = 0;
  // ---- settings, written only by mmda_misa_set_* (and mmda_misa_timing_stride / _rotate)
  // The optimizer's settings (mmda_misa_set_adam): every Adam launch of the handle reads them; scale_dev is not kept (a step with
  // clip_norm > 0 points its launches at gnorm[1]).  clip_norm > 0: clip_grad_norm_ in front of the update -- no update may precede the
  // norm, so such a step takes no early optimizer pass.
  mmda_adam_opts adam = {0.9f, 0.999f, 1e-8f, 0.f, 0, nullptr};
  float clip_norm = 0.f;
  // The classification criterion (mmda_misa_set_cls_loss): what every loss launch of the handle and the forward stretch's seed are
  // given (cls()); cls_on == 0: the plain one.  plan_step does not read it.
  mmda_cls_opts cls_opts = {}; int cls_on = 0;
  const mmda_cls_opts* cls() const { return cls_on ? &cls_opts : nullptr; }
  // The task (mmda_misa_set_task): REG_NONE (loss_terms.h) is the emotion classifier; REG_L1 / REG_MSE make the one output column a
  // regression output with that criterion, at the same sites that read cls().  plan_step does not read it either.
  int reg = REG_NONE;
  int fusion_fp8 = 0;
  int embed_update = EU_DENSE;
  // Frozen parameters (mmda_misa_set_trainable).  `runs`: the trainable ranges of the bucket, never merged across rnn2_begin, rnn1_begin
  // or embed -- so the runs of any range a launch of the step covers are a slice of the table -- and closed by an entry that carries the
  // table's item count.  A tensor's range runs up to the next tensor, alignment padding included.
  std::vector<mmda_run> runs;
  int prefix_frozen = 0;           // a tensor in front of the table is frozen
  int embed_flag = 1;              // the table's own flag (what embed_update makes of the table is a separate matter)
  int enc_frozen = 0;              // both recurrent layers and the three inter-layer LayerNorms are frozen
  int cut_keep_stash = 0;          // a cut step runs the stashing forward all the same (mmda_misa_set_cut_forward)
  // dense mode with deferral (mmda_misa_set_embed_deferred): the caller's per-row step counts and ring of step scalars (common.h:
  // DenseRowArgs).  Dense Adam's result; the bucket ends at the table as in the sparse mode, which also lends its pending rows.
  int32_t* df_row_step = nullptr; float* df_ring = nullptr; int df_window = 0;
  int use_side = 1;
  int use_cluster = 1;
  int use_bf16_gemm = 1;           // bf16 mode: LSTM-sized GEMMs read bf16 operand copies (gemm_bf16.hip)
  int inference = 0;               // evaluation passes: no stash, no copies that only the backward pass reads (a training step clears it)
  // Data-parallel "global statistics" mode (mmda_misa_set_external_batch_losses): the batch-statistic losses -- DiffLoss, CMD and the
  // confidence loss -- were computed by the caller on the batch of ALL ranks (all-gathered inputs, the same loss entry points), their
  // sums written into losses[1], [2], [4] and their gradient rows of THIS rank added into d_x6 / d_scores / d_tcp behind
  // mmda_misa_zero_act_grads: mmda_misa_losses then only adds what is a mean over samples (cls, recon) and the weighted total.
  int ext_batch_losses = 0;
  int ev_stride = 1;               // record every ev_stride-th step (the event pairs cost ~35 us per step)
  int ev_rotate = 0;               // 1: a sampled step brackets ONE of the four recurrent launches (sample index % 4): ~9 us
  // ---- device resources (created lazily, released by mmda_misa_destroy; no device memory but jflags and runs_dev)
  hipStream_t side = nullptr;      // second stream for weight-gradient GEMMs
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_pack = nullptr;
  hipEvent_t ev_early = nullptr;             // recorded by backward() when the gradients of the bucket prefix are final
  // The background pass over the embedding table (StepPlan::embed_bg).  A row the batch does not index has gradient zero, and its Adam
  // step needs nothing the step computes: a few workgroups on `bg`, a stream of the lowest priority, trickle that update under the
  // forward pass, where HBM is nearly idle, and the step's closing launch walks only the rows the batch does index.  Which rows those
  // are: row_stamp[V] on the device, where the launch that reads the step's ids writes bg_epoch (internal.h: RowStamp) -- padding
  // positions too, so the gather never reads a row the pass writes; no clear per step, the epoch moves on (all stamps are cleared
  // when it wraps to 0).  Fork: ev_bg_fork behind that launch, so the pass is ordered behind the stamps, the previous step and whatever
  // the caller queued.  Join: ev_bg_done, waited for by the side stream in front of the word it sets for the closing launch (flag
  // join), else by the main stream behind that launch.  All created at the first eligible step.
  hipStream_t bg = nullptr; hipEvent_t ev_bg_fork = nullptr, ev_bg_done = nullptr;
  unsigned* row_stamp = nullptr; unsigned bg_epoch = 0u;
  int bg_on = -1, bg_wgs = 0;                // mmda_misa_set_embed_background; -1 / 0: MMDA_EMBED_BG's / MMDA_EMBED_BG_WGS's (else the default)
  // (the pass's workgroups hold LDS they never touch, MMDA_EMBED_BG_LDS bytes: a resident recurrence reserves the whole LDS of its CUs,
  //  so the two never share a CU -- sharing one cost each forward recurrence 24 us of its hand-offs at any throttle)
  int bg_pending = 0, bg_active = 0;         // the pass went out and is not joined yet; the last train_step ran it
  // Flag joins (training step; common.h: flag_wait): where the main stream needs a side-stream chain's results, the consuming KERNEL
  // waits on the device for a word that a one-thread launch behind the chain sets, instead of the stream waiting for an event -- an
  // event wait costs the main stream 9 - 12 us of packet processing even when the chain finished long ago (tools/micro/fork_cost.hip),
  // twice per step.  Forward: the loss chain's gradients (d_x6) are first read by the LayerNorm-1 stretch of the backward pass
  // (fused_bwd_a_kernel).  Backward: nothing on the main stream reads what the side stream's weight-gradient GEMMs and early
  // optimizer pass write; the step's last optimizer launch simply does not complete before they have.  ev_join is still recorded
  // behind each chain for the paths that cannot wait on the device.  MMDA_FLAG_JOIN=0: event joins as before.
  unsigned* jflags = nullptr;                // device: [0] forward chain done, [1] backward chain done, [2] a wait timed out, [3] id list sorted
  // runs_dev: the table of trainable runs on the device (the one allocation besides jflags), copied when the set has changed since
  // the last launch that read it.
  mmda_run* runs_dev = nullptr; int runs_dev_cap = 0; int runs_dirty = 1;
  // optional per-launch timing of the four recurrent kernels (bench.py roofline leg)
  std::vector<hipEvent_t> ev;      // [step][slot][start/stop]
  // ---- the state of the step in flight
  StepPlan plan;                             // its decisions (plan_step)
  int64_t early_floats = 0; int early_valid = 0;
  // fused train step without a gradient exchange: clamp+Adam of the bucket prefix whose gradients are final beside the layer-1 backward
  // recurrence runs there, on the side stream (Pass::opt); how far that pass of the last backward got
  int64_t adam_early_done = 0;
  int wT_valid = 0;                // the K-major fusion-weight copies in the workspace are this step's
  int wT_pending = 0;              // the K-major fusion-weight copies of this step are still to be made (on the next fork)
  // sparse mode, backward without an optimizer step behind it (do_adam = 0, the autograd path): the pass stops at d_x_t and
  // mmda_misa_adam_step applies the rows update from the id list / lengths of that backward (the caller keeps them alive, as it does
  // for backward itself)
  PendingRows eu;
  // deferred table: df_seq: updates applied since the binding (what a current row's row_step equals); df_flushed: df_seq at the last full flush.
  int df_seq = 0, df_flushed = 0;
  // state of the last forward (dropout replay in backward)
  int training = 0; uint64_t seed = 0;
  unsigned epoch = 1;              // monotonic cluster-exchange epoch (never reset; see lstm_resident.h)
  int side_pending = 0;
  int zero_grad_pending = 0;       // train_step: the gradient bucket is cleared inside forward(), beside the fusion block
  // train_step (StepPlan::fused): the losses that read only the private/shared representations (diff, CMD) are issued by forward() on
  // the side stream as soon as those exist, beside the transformer layer and the heads; mmda_misa_losses() then adds the rest
  int eager_done = 0;                        // that chain, and any loss seeds, not yet taken up by mmda_misa_losses
  // Loss seeds (training step, fused row-local stretches): the forward stretches store the gradient seeds of the reconstruction loss
  // (d_recon, d_orig) and -- without ConfidNet, whose loss adds into the same buffer -- of the classification loss (d_scores) where
  // they produce recon / scores, so the launch that computes cls / conf / recon and the weighted total has no gradient to seed and
  // leaves the critical path between the forward and the backward pass (14 us at B=32): it runs on the side stream beside the
  // layer-2 backward recurrence.  Values are bit-identical to the loss launch's (same expressions on the same operands).
  const float* misc_deferred = nullptr;      // labels: the loss-value launch is still to be issued (backward's first side fork)
  unsigned jval[2] = {0u, 0u};               // the values the flag-join words [0], [1] were last set to
  // The sort-based embedding scatter of a large batch in two halves: the sorted (id, position) list depends on the ids only and is
  // made on the side stream beside the layer-2 backward recurrence (33 us of launches at B=256 that used to sit between the last
  // GEMM and the optimizer); word [3] tells the main stream it is there (a one-wave wait launch in front of the sums).
  int esort_valid = 0; unsigned esort_val = 0u;
  int fj1 = 0, fj2 = 0, fj1_armed = 0;
  int ev_steps = 0, ev_fwd = 0, ev_bwd = 0;
  int ev_seen_f = 0, ev_seen_b = 0;
  std::vector<char> ev_done;                         // (step, slot) was recorded

 private:
  Workspace lay_{};
};

namespace {

// ---------------------------------------------------------------------------------------------- GEMM shorthands
struct Ctx {
  mmda_misa* m; void* s; int rc = 0;
  bool grouping = false; std::vector<mmda_gemm_args> pending;
  bool absent_next = false; std::vector<mmda_gemm_args> absent;   // a product the step leaves out, still counted when the group is sized
  bool deferring = false; std::vector<mmda_gemm_args> deferred;   // weight-gradient GEMMs: off the critical path, run on the side stream
};

// independent GEMMs issued between group_begin/group_end go out as ONE grouped launch
void group_begin(Ctx& c) { c.grouping = true; c.pending.clear(); c.absent.clear(); }
void group_end(Ctx& c) {
  c.grouping = false;
  if (!c.rc && !c.pending.empty())
    c.rc = mmda_gemm_grouped_sized(c.pending.data(), (int)c.pending.size(), c.absent.data(), (int)c.absent.size(), c.s);
  c.pending.clear(); c.absent.clear();
}

void gemm(Ctx& c, int mode, int tA, int tB, int M, int N, int K, const float* A, int lda, const float* Bp, int ldb, float* C,
          int ldc, const float* bias = nullptr, const float* bias2 = nullptr, int acc = 0, int act = 0, int batch = 1,
          int64_t sA = 0, int64_t sB = 0, int64_t sC = 0, int64_t sBias = 0, mmda_gemm_args* extra = nullptr) {
  if (c.rc) return;
  mmda_gemm_args g = {};
  if (extra) g = *extra;
  g.mode = mode; g.transA = tA; g.transB = tB; g.M = M; g.N = N; g.K = K; g.batch = batch;
  g.A = A; g.lda = lda; g.strideA = sA; g.B = Bp; g.ldb = ldb; g.strideB = sB; g.C = C; g.ldc = ldc; g.strideC = sC;
  g.bias = bias; g.bias2 = bias2; g.strideBias = sBias; g.accumulate = acc; g.act = act;
  if (c.absent_next) { c.absent_next = false; if (c.grouping) c.absent.push_back(g); return; }
  if (c.deferring && tA && acc) c.deferred.push_back(g);       // TN + accumulate == a weight gradient
  else if (c.grouping) c.pending.push_back(g);
  else c.rc = mmda_gemm(&g, c.s);
}

// Fork/join with the side stream: everything in `list` only has to be finished before the optimizer step, so it runs
// concurrently with the recurrent kernels (which occupy ~10 % of the CUs while they walk the serial chain).
int side_fork(mmda_misa* m, void* main_stream, void** out);
int side_launch(mmda_misa* m, std::vector<mmda_gemm_args>& list, void* main_stream);
int side_join(mmda_misa* m, void* main_stream);
// y(M,N) = x(M,K) W(N,K)^T + b
void lin_fwd(Ctx& c, int mode, int M, int N, int K, const float* x, const float* W, const float* b, float* y, int act = 0) {
  gemm(c, mode, 0, 1, M, N, K, x, K, W, K, y, N, b, nullptr, 0, act);
}
// dx(M,K) (+)= dy(M,N) W(N,K)
void lin_dx(Ctx& c, int mode, int M, int N, int K, const float* dy, const float* W, float* dx, int acc) {
  gemm(c, mode, 0, 0, M, K, N, dy, N, W, K, dx, K, nullptr, nullptr, acc);
}
// dW(N,K) += dy(M,N)^T x(M,K);  db(N) += colsum(dy)
void lin_dw(Ctx& c, int mode, int M, int N, int K, const float* dy, const float* x, float* dW, float* db) {
  mmda_gemm_args e = {};
  e.bias_grad = db;                 // the bias gradient rides along as a virtual ones-column of the same GEMM
  gemm(c, mode, 1, 0, N, K, M, dy, N, x, K, dW, K, nullptr, nullptr, 1, 0, 1, 0, 0, 0, 0, &e);
}

// ---- row-skinny forms (fusion block at B <= SKINNY_MAX_B): see gemm_skinny.hip
// y(M,N) = act(x(M,K) W(N,K)^T + b)
mmda_skinny_args sk_nt(int M, int N, int K, const float* x, int ldx, const float* W, const float* b, float* y, int ldy, int act = 0) {
  mmda_skinny_args g = {};
  g.M = M; g.N = N; g.K = K; g.transB = 1; g.A = x; g.lda = ldx; g.B = W; g.ldb = K; g.C = y; g.ldc = ldy; g.bias = b; g.act = act;
  return g;
}
// dx(M,K) (+)= dy(M,N) W(N,K)
mmda_skinny_args sk_nn(int M, int N, int K, const float* dy, int lddy, const float* W, float* dx, int lddx, int acc) {
  mmda_skinny_args g = {};
  g.M = M; g.N = K; g.K = N; g.transB = 0; g.A = dy; g.lda = lddy; g.B = W; g.ldb = K; g.C = dx; g.ldc = lddx; g.accumulate = acc;
  return g;
}
// dx(M,K) (+)= dy(M,N) W(N,K) through the K-major copy WT(K,N): an NT problem (float4 loads along the reduction for both operands)
mmda_skinny_args sk_dx(int M, int N, int K, const float* dy, int lddy, const float* WT, float* dx, int lddx, int acc) {
  mmda_skinny_args g = {};
  g.M = M; g.N = K; g.K = N; g.transB = 1; g.A = dy; g.lda = lddy; g.B = WT; g.ldb = N; g.C = dx; g.ldc = lddx; g.accumulate = acc;
  return g;
}
// ... through WT where this step made the K-major copy (wt), else through W as it lies
mmda_skinny_args sk_dxw(bool wt, int M, int N, int K, const float* dy, int lddy, const float* WT, const float* W, float* dx, int lddx,
                        int acc) {
  return wt ? sk_dx(M, N, K, dy, lddy, WT, dx, lddx, acc) : sk_nn(M, N, K, dy, lddy, W, dx, lddx, acc);
}
void sk_launch(Ctx& c, const mmda_skinny_args* p, int n) {
  if (!c.rc) c.rc = mmda_gemm_skinny(p, n, c.s);
}


void ev_rec(mmda_misa* m, int step, int slot, int which, void* stream) {
  if (m->ev.empty() || step >= m->ev_steps) return;
  if ((slot < 2 ? m->ev_seen_f : m->ev_seen_b) % m->ev_stride) return;
  if (m->ev_rotate && slot != (step & 3)) return;
  (void)hipEventRecord(m->ev[(step * 4 + slot) * 2 + which], (hipStream_t)stream);
  if (which == 1 && (size_t)(step * 4 + slot) < m->ev_done.size()) m->ev_done[step * 4 + slot] = 1;
}

// Fork: work issued on the returned stream starts after everything already on `main_stream` and runs beside what follows
// there; side_join() makes `main_stream` wait for it.  Without overlap the main stream itself is returned.
unsigned fork_event_flags() {
  static const int sysfence = mmda_env_int("MMDA_EVENT_SYSFENCE", 0);
  return hipEventDisableTiming | (sysfence ? 0u : hipEventDisableSystemFence);
}
int side_fork(mmda_misa* m, void* main_stream, void** out) {
  *out = main_stream;
  if (!m->use_side) return MMDA_OK;
  if (!m->side) {
    if (hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking) != hipSuccess) return MMDA_ELAUNCH;
    // The fork / join events order streams of ONE device: no system-scope fence with them (hipEventDisableSystemFence -- "device
    // memory may not be visible to the host and other devices", neither of which waits on these events; every kernel still ends with
    // its own device-scope release).  With the fence a recorded event costs the recording stream 6 us between two launches, without
    // it 3 (tools/micro/fork_cost.hip).  MMDA_EVENT_SYSFENCE=1: with the fence.
    const unsigned evf = fork_event_flags();
    if (hipEventCreateWithFlags(&m->ev_fork, evf) != hipSuccess) return MMDA_ELAUNCH;
    if (hipEventCreateWithFlags(&m->ev_join, evf) != hipSuccess) return MMDA_ELAUNCH;
    if (hipEventCreateWithFlags(&m->ev_pack, evf) != hipSuccess) return MMDA_ELAUNCH;
    if (hipMalloc(reinterpret_cast<void**>(&m->jflags), 64) != hipSuccess) { m->jflags = nullptr; return MMDA_ELAUNCH; }
    if (hipMemset(m->jflags, 0, 64) != hipSuccess) return MMDA_ELAUNCH;
  }
  if (hipEventRecord(m->ev_fork, (hipStream_t)main_stream) != hipSuccess) return MMDA_ELAUNCH;
  if (hipStreamWaitEvent(m->side, m->ev_fork, 0) != hipSuccess) return MMDA_ELAUNCH;
  m->side_pending = 1;
  *out = m->side;
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
__global__ void flag_wait_kernel(const unsigned* flag, unsigned value, unsigned* err) { flag_wait(flag, value, err); }
__global__ void flag_set_kernel(unsigned* flag, unsigned value) {
  __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// the side stream's chain ends here for the main stream: word `idx` is set behind it (flag join) -- or was, by the chain's last launch
// itself (by_kernel) --; ev_join is recorded too
int side_flag_signal(mmda_misa* m, int idx, bool by_kernel = false) {
  if (!m->side || !m->jflags) return MMDA_EINVAL;
  ++m->jval[idx];
  if (!by_kernel) {
    hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(1), 0, m->side, m->jflags + idx, m->jval[idx]);
    MMDA_CHECK_LAUNCH("side_flag_signal");
  }
  if (hipEventRecord(m->ev_join, m->side) != hipSuccess) return MMDA_ELAUNCH;
  m->side_pending = 0;
  return MMDA_OK;
}
// a flag join whose consumer kernel will not run after all: the event recorded with it
int flag_join_fallback(mmda_misa* m, void* main_stream) {
  if (hipStreamWaitEvent((hipStream_t)main_stream, m->ev_join, 0) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}
int side_join(mmda_misa* m, void* main_stream) {
  if (!m->side_pending) return MMDA_OK;
  if (hipEventRecord(m->ev_join, m->side) != hipSuccess) return MMDA_ELAUNCH;
  if (hipStreamWaitEvent((hipStream_t)main_stream, m->ev_join, 0) != hipSuccess) return MMDA_ELAUNCH;
  m->side_pending = 0;
  return MMDA_OK;
}

// ---- the background pass over the embedding table (see mmda_misa::bg)
// Its stream, events and stamps, made once; then the step's epoch.  What the launch that reads the n ids stamps with: *st.
int bg_begin(mmda_misa* m, const int64_t* ids, int n, void* main_stream, RowStamp* st) {
  const size_t bytes = sizeof(unsigned) * (size_t)m->cfg.vocab;
  if (!m->bg) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return MMDA_ELAUNCH;
    if (hipStreamCreateWithPriority(&m->bg, hipStreamNonBlocking, least) != hipSuccess) { m->bg = nullptr; return MMDA_ELAUNCH; }
    if (hipEventCreateWithFlags(&m->ev_bg_fork, fork_event_flags()) != hipSuccess) return MMDA_ELAUNCH;
    if (hipEventCreateWithFlags(&m->ev_bg_done, fork_event_flags()) != hipSuccess) return MMDA_ELAUNCH;
  }
  if (!m->row_stamp) {
    if (hipMalloc(reinterpret_cast<void**>(&m->row_stamp), bytes) != hipSuccess) { m->row_stamp = nullptr; return MMDA_ELAUNCH; }
    if (hipMemset(m->row_stamp, 0, bytes) != hipSuccess) return MMDA_ELAUNCH;
    m->bg_epoch = 0u;
  }
  if (!m->ev_bg_fork || !m->ev_bg_done) return MMDA_ELAUNCH;
  if (++m->bg_epoch == 0u) {                             // wrapped: a stamp of 2^32 steps ago would read as this step's
    if (hipMemsetAsync(m->row_stamp, 0, bytes, (hipStream_t)main_stream) != hipSuccess) return MMDA_ELAUNCH;
    m->bg_epoch = 1u;
  }
  *st = RowStamp{m->row_stamp, m->bg_epoch, m->cfg.vocab, ids, n};
  return MMDA_OK;
}
TableRows bg_table(const mmda_misa* m) { return TableRows{m->row_stamp, m->bg_epoch, m->cfg.vocab, m->cfg.d_t}; }
AdamHyper bg_hyper(const mmda_misa* m, const OptStep& o) {
  return AdamHyper{o.lr, m->adam.beta1, m->adam.beta2, m->adam.eps, o.clip, o.grad_scale, o.step, m->adam.weight_decay, m->adam.decoupled, nullptr};
}
// the fork and the pass (the step's optimizer step: `opt`): behind everything `main_stream` holds
int bg_launch(mmda_misa* m, const OptStep* opt, void* main_stream) {
  if (!opt || !m->bg || !m->row_stamp) return MMDA_EINVAL;
  if (hipEventRecord(m->ev_bg_fork, (hipStream_t)main_stream) != hipSuccess) return MMDA_ELAUNCH;
  if (hipStreamWaitEvent(m->bg, m->ev_bg_fork, 0) != hipSuccess) return MMDA_ELAUNCH;
  const int64_t e = m->par.embed;
  const int rc = mmda_adam_background_launch(m->P + e, m->M1 + e, m->V1 + e, bg_table(m), bg_hyper(m, *opt), m->plan.embed_bg_wgs,
                                             m->plan.embed_bg_lds, m->bg);
  if (rc) return rc;
  m->bg_pending = 1; m->bg_active = 1;                   // (from here on rows may have taken the step, whatever the step returns)
  if (hipEventRecord(m->ev_bg_done, m->bg) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}
// join: `stream` (the side stream in front of its flag word, or the main stream) goes on only when the pass is through
int bg_join(mmda_misa* m, void* stream) {
  if (!m->bg_pending) return MMDA_OK;
  if (hipStreamWaitEvent((hipStream_t)stream, m->ev_bg_done, 0) != hipSuccess) return MMDA_ELAUNCH;
  m->bg_pending = 0;
  return MMDA_OK;
}

#define WS(off) (m->ws + (off))
#define PP(off) (m->P + (off))
#define GG(off) (m->G + (off))

// Recurrent-layer parameters / gradients as the kernels see them: the bound flat buffers (LSTM) or the four-slot workspace
// copies (GRU; filled by mmda_gru_pad_params at the top of forward, folded back by mmda_gru_unpad_grads at the end of backward).
inline bool is_gru(const mmda_misa* m) { return m->cfg.rnncell == MMDA_CELL_GRU; }
inline float* rW_ih(mmda_misa* m, int i, int l) { return is_gru(m) ? WS(m->lay.mod[i].rnn[l].pw_ih) : PP(m->par.mod[i].rnn[l].w_ih); }
inline float* rW_hh(mmda_misa* m, int i, int l, int d) { return is_gru(m) ? WS(m->lay.mod[i].rnn[l].pw_hh[d]) : PP(m->par.mod[i].rnn[l].w_hh[d]); }
inline float* rB_ih(mmda_misa* m, int i, int l) { return is_gru(m) ? WS(m->lay.mod[i].rnn[l].pb_ih) : PP(m->par.mod[i].rnn[l].b_ih); }
inline float* rB_hh(mmda_misa* m, int i, int l) { return is_gru(m) ? WS(m->lay.mod[i].rnn[l].pb_hh) : PP(m->par.mod[i].rnn[l].b_hh); }
inline float* gW_ih(mmda_misa* m, int i, int l) { return is_gru(m) ? WS(m->lay.mod[i].rnn[l].gw_ih) : GG(m->par.mod[i].rnn[l].w_ih); }
inline float* gW_hh(mmda_misa* m, int i, int l, int d) { return is_gru(m) ? WS(m->lay.mod[i].rnn[l].gw_hh[d]) : GG(m->par.mod[i].rnn[l].w_hh[d]); }
inline float* gB_ih(mmda_misa* m, int i, int l) { return is_gru(m) ? WS(m->lay.mod[i].rnn[l].gb) : GG(m->par.mod[i].rnn[l].b_ih); }
inline float* gB_hh(mmda_misa* m, int i, int l) { return is_gru(m) ? nullptr : GG(m->par.mod[i].rnn[l].b_hh); }

// GRU: jobs for the pad / unpad kernels; `base` is the flat parameter (pad) or gradient (unpad) buffer
int gru_jobs(mmda_misa* m, float* base, bool grads, mmda_gru_pad_job* j) {
  int n = 0;
  for (int i = 0; i < 3; ++i)
    for (int l = 0; l < 2; ++l, ++n) {
      const RnnP& r = m->par.mod[i].rnn[l]; const RnnW& rw = m->lay.mod[i].rnn[l];
      j[n] = mmda_gru_pad_job{};
      j[n].H = r.H; j[n].D = r.D;
      for (int d = 0; d < 2; ++d) {
        j[n].w_ih[d] = base + r.w_ih + (int64_t)d * 3 * r.H * r.D; j[n].w_hh[d] = base + r.w_hh[d];
        j[n].b_ih[d] = base + r.b_ih + (int64_t)d * 3 * r.H; j[n].b_hh[d] = base + r.b_hh + (int64_t)d * 3 * r.H;
        j[n].pw_hh[d] = grads ? WS(rw.gw_hh[d]) : WS(rw.pw_hh[d]);
      }
      j[n].pw_ih = grads ? WS(rw.gw_ih) : WS(rw.pw_ih);
      j[n].pb_ih = grads ? WS(rw.gb) : WS(rw.pb_ih);
      j[n].pb_hh = grads ? nullptr : WS(rw.pb_hh);
    }
  return n;
}

// parameters of a parametrised activation (prelu / rrelu) at one of its uses; zeros for every other activation
mmda_act_params act_params(mmda_misa* m, int training, uint64_t seed, int site, bool grads) {
  mmda_act_params p = {};
  if (m->cfg.act == MMDA_ACT_PRELU) { p.slope = m->P + m->par.prelu_a; p.dslope = grads ? m->G + m->par.prelu_a : nullptr; }
  if (m->cfg.act == MMDA_ACT_RRELU) { p.lo = 1.0f / 8.0f; p.hi = 1.0f / 3.0f; p.rand = training ? 1 : 0; p.seed = seed; p.site = site; }   // torch defaults
  return p;
}

int check_ready(const mmda_misa* m) {
  if (!m || !m->P || !m->ws) return MMDA_EINVAL;
  return MMDA_OK;
}

// recurrent descriptor of modality i, layer l: forward (W_hh packed for the forward kernels, utt) or backward (streaming backward
// packing, the resident-weights one where `with_c`, d_utt, d(hseq of layer 1))
mmda_lstm_desc lstm_desc(mmda_misa* m, int i, int l, bool bwd, int gate_minor, bool with_c) {
  const ModW& mw = m->lay.mod[i]; const RnnW& rw = mw.rnn[l];
  const int64_t* wp = bwd ? rw.pack_b : rw.pack_f;
  mmda_lstm_desc d = {};
  d.H = m->par.mod[i].rnn[l].H; d.gates = WS(mw.gates[l]); d.cstash = WS(mw.c[l]); d.hseq = WS(mw.hseq[l]);
  d.wpack[0] = WS(wp[0]); d.wpack[1] = WS(wp[1]);
  if (with_c) { d.wpack_c[0] = WS(rw.pack_c[0]); d.wpack_c[1] = WS(rw.pack_c[1]); }
  d.utt = WS(bwd ? mw.d_utt : mw.utt); d.layer = l; d.d_hseq = bwd && l == 0 ? WS(mw.d_hseq1) : nullptr;
  d.xchg = (m->use_cluster && mw.xchg >= 0) ? (void*)WS(mw.xchg) : nullptr; d.epoch_base = m->epoch;
  d.gate_minor = gate_minor; d.cell = m->cfg.rnncell;
  return d;
}

// floats of the gradient bucket that a step writes, clears and walks with dense Adam: all of it, or the prefix in front of the table
int64_t grad_floats(const mmda_misa* m) { return m->embed_update == EU_DENSE && !m->df_row_step ? m->par.flat : m->par.embed; }

// ---- frozen parameters
// a launch over [0, grad_floats) has a frozen float to leave out (else the step is today's: the dense kernels, the early pass)
bool masked(const mmda_misa* m) { return m->prefix_frozen || (!m->embed_flag && grad_floats(m) == m->par.flat); }
// the encoder cut: nothing behind the fusion block trains -- the recurrent layers and the inter-layer LayerNorms are frozen and the
// table is, by its flag (dense) or by embed_update (the sparse and deferred modes train the table through d_x: no cut)
bool encoder_cut(const mmda_misa* m) {
  return m->enc_frozen && (m->embed_update == EU_FROZEN || (m->embed_update == EU_DENSE && !m->df_row_step && !m->embed_flag));
}
// the table's slice for the bucket range [lo, hi), both of them 0, rnn2_begin, rnn1_begin, embed or flat
void runs_slice(const mmda_misa* m, int64_t lo, int64_t hi, int* r0, int* n, int64_t* items) {
  const int nr = (int)m->runs.size() - 1;
  int a = 0;
  while (a < nr && m->runs[a].begin < lo) ++a;
  int b = a;
  while (b < nr && m->runs[b].begin < hi) ++b;
  *r0 = a; *n = b - a; *items = m->runs[b].first - m->runs[a].first;
}
// the table on the device, current.  A changed set waits for the streams that may still read the old table: once per change.
int runs_ready(mmda_misa* m, void* stream) {
  if (!m->runs_dirty && m->runs_dev) return MMDA_OK;
  const int need = (int)m->runs.size();
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return MMDA_ELAUNCH;
  if (m->side && hipStreamSynchronize(m->side) != hipSuccess) return MMDA_ELAUNCH;
  if (need > m->runs_dev_cap) {
    if (m->runs_dev) (void)hipFree(m->runs_dev);
    m->runs_dev = nullptr; m->runs_dev_cap = 0;
    const int cap = (int)m->par.params.size() + 1;            // every tensor a run of its own, and the closing entry
    if (hipMalloc(reinterpret_cast<void**>(&m->runs_dev), sizeof(mmda_run) * cap) != hipSuccess) { m->runs_dev = nullptr; return MMDA_ELAUNCH; }
    m->runs_dev_cap = cap;
  }
  if (hipMemcpy(m->runs_dev, m->runs.data(), sizeof(mmda_run) * need, hipMemcpyHostToDevice) != hipSuccess) return MMDA_ELAUNCH;
  m->runs_dirty = 0;
  return MMDA_OK;
}
// The model's Adam unless mmda_misa_set_adam says otherwise (the reference gives torch.optim.Adam nothing but lr)
constexpr mmda_adam_opts kAdamDefaults = {0.9f, 0.999f, 1e-8f, 0.f, 0, nullptr};
// clamp + Adam over the bucket range [lo, hi) with the gradient G, or acc + G (acc != nullptr: the accumulator, laid out like the
// bucket): the dense stream, or -- frozen parameters -- the trainable runs of that range, where a range with nothing to train launches
// nothing but for a waiter (w.flag != nullptr).
// scale_dev: the clip coefficient of a step with clip_norm > 0 (bucket_norm below), else nullptr.
int bucket_adam(mmda_misa* m, int64_t lo, int64_t hi, const float* acc, float lr, float clip, float grad_scale, int step, const FlagWait& w,
                void* stream, const float* scale_dev = nullptr) {
  const AdamHyper h{lr, m->adam.beta1, m->adam.beta2, m->adam.eps, clip, grad_scale, step, m->adam.weight_decay, m->adam.decoupled, scale_dev};
  if (!masked(m)) return mmda_adam_launch(m->P + lo, acc ? acc + lo : nullptr, m->G + lo, m->M1 + lo, m->V1 + lo, hi - lo, nullptr, h, w, stream);
  int r0 = 0, n = 0; int64_t items = 0;
  runs_slice(m, lo, hi, &r0, &n, &items);
  if (n > 0 && (m->runs_dirty || !m->runs_dev)) return MMDA_EINVAL;      // (every entry that gets here called runs_ready first)
  const RunTable t{n > 0 ? m->runs_dev + r0 : nullptr, n, items};
  return mmda_adam_launch(m->P, acc, m->G, m->M1, m->V1, 0, &t, h, w, stream);
}
// clip_norm > 0: the norm of the gradient the step is about to apply -- G or acc + G over [0, grad_floats), the trainable runs of it
// when parameters are frozen -- and the clip coefficient, into gnorm[0], gnorm[1]
int bucket_norm(mmda_misa* m, const float* acc, float grad_scale, void* stream) {
  if (!m->ws || m->lay.gnorm < 0) return MMDA_EINVAL;
  double* parts = reinterpret_cast<double*>(m->ws + m->lay.gnorm_parts);
  const int64_t cap = mmda_grad_norm_partials(INT64_MAX);
  const int64_t hi = grad_floats(m);
  if (!masked(m)) return mmda_grad_norm_launch(m->G, acc, hi, nullptr, m->clip_norm, grad_scale, parts, cap, m->ws + m->lay.gnorm, stream);
  int r0 = 0, n = 0; int64_t items = 0;
  runs_slice(m, 0, hi, &r0, &n, &items);
  if (n > 0 && (m->runs_dirty || !m->runs_dev)) return MMDA_EINVAL;
  const RunTable t{n > 0 ? m->runs_dev + r0 : nullptr, n, items};
  return mmda_grad_norm_launch(m->G, acc, 0, &t, m->clip_norm, grad_scale, parts, cap, m->ws + m->lay.gnorm, stream);
}
// what no step does (checked in front of its first launch, so a refused call changes nothing): decay under the deferred table -- the
// replay ring holds two scalars per update, a decayed zero-gradient step needs a third; a norm clip with a table whose rows are updated
// where their sums become final, before a norm exists
bool adam_settings_refused(const mmda_misa* m) {
  if (m->adam.weight_decay > 0.f && m->df_row_step) return true;
  if (m->clip_norm > 0.f && (m->embed_update == EU_SPARSE || m->df_row_step)) return true;
  return false;
}
// the table from one flag per parameter (nullptr: everything trains)
int apply_trainable(mmda_misa* m, const unsigned char* flags) {
  const int np = (int)m->par.params.size();
  std::vector<int64_t> begin, len;
  int prefix_frozen = 0, embed_flag = 1, enc_frozen = 1;
  for (int i = 0; i < np; ++i) {
    const ParamInfo& p = m->par.params[i];
    const bool on = !flags || flags[i] != 0;
    const std::string top = p.name.substr(0, p.name.find('.'));
    if (p.off == m->par.embed) embed_flag = on ? 1 : 0;
    else if (!on) prefix_frozen = 1;
    if (on && ((p.off >= m->par.rnn2_begin && p.off < m->par.embed) || top == "tlayer_norm" || top == "vlayer_norm" || top == "alayer_norm")) enc_frozen = 0;
    if (!on) continue;
    begin.push_back(p.off);
    len.push_back((i + 1 < np ? m->par.params[i + 1].off : m->par.flat) - p.off);
  }
  const int64_t cuts[3] = {m->par.rnn2_begin, m->par.rnn1_begin, m->par.embed};
  std::vector<mmda_run> runs(begin.size() + 1);
  int n = 0;
  const int64_t items = mmda_runs_build_cut(begin.data(), len.data(), (int)begin.size(), m->par.flat, cuts, 3, runs.data(), &n);
  if (items < 0) return MMDA_EINVAL;
  runs.resize(n + 1);
  runs[n] = mmda_run{m->par.flat, 0, items};
  m->runs.swap(runs);
  m->prefix_frozen = prefix_frozen; m->embed_flag = embed_flag; m->enc_frozen = enc_frozen;
  m->runs_dirty = 1;
  return MMDA_OK;
}

// the process's switches that select a form of the step: read here, once, and nowhere else in this file
const StepSwitches& step_switches() {
  static const StepSwitches d, sw = {
      mmda_env_int("MMDA_GEMM_TN", d.gemm_tn), mmda_env_int("MMDA_WT_MERGE", d.wt_merge), mmda_env_int("MMDA_ROW_FUSE", d.row_fuse),
      mmda_env_int("MMDA_FFN_FUSE", d.ffn_fuse), mmda_env_int("MMDA_LOSS_SEEDS", d.loss_seeds), mmda_env_int("MMDA_FLAG_JOIN", d.flag_join),
      mmda_env_int("MMDA_ZERO_GRAD_SIDE", d.zero_grad_side), mmda_env_int("MMDA_FUSED_SPLIT", d.fused_split),
      mmda_env_int("MMDA_SORT_EARLY", d.sort_early), mmda_env_int("MMDA_EMBED_BG", d.embed_bg), mmda_env_int("MMDA_EMBED_BG_WGS", d.embed_bg_wgs),
      mmda_env_int("MMDA_EMBED_BG_LATE", d.embed_bg_late), mmda_env_int("MMDA_EMBED_BG_LDS", d.embed_bg_lds)};
  return sw;
}
// what plan_step is given for a pass over (B, T) batches: the handle's settings and the request, as values
PlanInput plan_input(const mmda_misa* m, const StepRequest& r, int B, int T) {
  PlanInput in = {};
  in.cfg = m->cfg; in.B = B; in.T = T;
  for (int i = 0; i < 3; ++i) { in.H[i] = m->par.mod[i].H; in.xchg[i] = mmda_lstm_xchg_bytes(in.H[i], B) > 0; }
  in.use_side = m->use_side != 0; in.use_cluster = m->use_cluster != 0; in.use_bf16_gemm = m->use_bf16_gemm != 0;
  in.inference = m->inference != 0; in.fusion_fp8 = m->fusion_fp8 != 0;
  in.embed_update = m->embed_update; in.embed_deferred = m->embed_update == EU_DENSE && m->df_row_step != nullptr;
  in.masked = masked(m); in.encoder_cut = encoder_cut(m); in.cut_keep_stash = m->cut_keep_stash != 0;
  in.bg_on = m->bg_on; in.bg_wgs = m->bg_wgs; in.moments = m->M1 && m->V1;
  in.fused = r.fused; in.has_labels = r.emo != nullptr; in.has_opt = r.opt != nullptr; in.enc_cached = r.enc_cached;
  return in;
}

}  // namespace

// =============================================================================================== lifecycle
extern "C" int mmda_misa_create(const mmda_misa_config* cfg, mmda_misa** out) {
  if (!cfg || !out) return MMDA_EINVAL;
  if (cfg->vocab <= 0 || cfg->d_t <= 0 || cfg->d_v <= 0 || cfg->d_a <= 0 || cfg->hidden <= 0 || cfg->ncls <= 0) return MMDA_EINVAL;
  if (cfg->d_t > 512 || cfg->d_v > 512 || cfg->d_a > 512 || cfg->hidden % NHEAD || cfg->hidden > 1024) return MMDA_EINVAL;
  if (cfg->mode != MMDA_F32 && cfg->mode != MMDA_BF16) return MMDA_EINVAL;
  if (cfg->rnncell != MMDA_CELL_LSTM && cfg->rnncell != MMDA_CELL_GRU) return MMDA_EINVAL;
  mmda_misa* m = new mmda_misa(*cfg);
  if (apply_trainable(m, nullptr)) { delete m; return MMDA_EINVAL; }
  *out = m;
  return MMDA_OK;
}
extern "C" void mmda_misa_destroy(mmda_misa* m) {
  if (!m) return;
  if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
  if (m->ev_join) (void)hipEventDestroy(m->ev_join);
  if (m->ev_pack) (void)hipEventDestroy(m->ev_pack);
  if (m->ev_early) (void)hipEventDestroy(m->ev_early);
  if (m->bg) { (void)hipStreamSynchronize(m->bg); (void)hipStreamDestroy(m->bg); }
  if (m->ev_bg_fork) (void)hipEventDestroy(m->ev_bg_fork);
  if (m->ev_bg_done) (void)hipEventDestroy(m->ev_bg_done);
  if (m->row_stamp) (void)hipFree(m->row_stamp);
  if (m->side) (void)hipStreamDestroy(m->side);
  if (m->jflags) (void)hipFree(m->jflags);
  if (m->runs_dev) (void)hipFree(m->runs_dev);
  for (hipEvent_t e : m->ev) (void)hipEventDestroy(e);
  delete m;
}
extern "C" int mmda_misa_num_params(const mmda_misa* m) { return m ? (int)m->par.params.size() : MMDA_EINVAL; }
extern "C" int mmda_misa_param_info(const mmda_misa* m, int i, const char** name, int64_t* offset, int* rows, int* cols) {
  if (!m || i < 0 || i >= (int)m->par.params.size()) return MMDA_EINVAL;
  const ParamInfo& p = m->par.params[i];
  if (name) *name = p.name.c_str();
  if (offset) *offset = p.off;
  if (rows) *rows = p.rows;
  if (cols) *cols = p.cols;
  return MMDA_OK;
}
extern "C" int64_t mmda_misa_flat_floats(const mmda_misa* m) { return m ? m->par.flat : MMDA_EINVAL; }
extern "C" int64_t mmda_misa_dense_floats(const mmda_misa* m) { return m ? m->par.dense : MMDA_EINVAL; }
extern "C" int mmda_misa_bind(mmda_misa* m, float* params, float* grads, float* adam_m, float* adam_v) {
  if (!m || !params) return MMDA_EINVAL;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)adam_m | (uintptr_t)adam_v) & 15) return MMDA_EINVAL;
  m->P = params; m->G = grads; m->M1 = adam_m; m->V1 = adam_v;
  return MMDA_OK;
}
extern "C" int64_t mmda_misa_workspace_floats(const mmda_misa* m, int B, int T) {
  if (!m || B <= 0 || T <= 0) return MMDA_EINVAL;
  return carve(m->cfg, m->par, B, T).floats;
}
// The plan a forward pass over (B, T) batches would get: host only, no workspace needed, the switches given instead of read
extern "C" int mmda_misa_plan_describe(const mmda_misa* m, int B, int T, const mmda_misa_step_request* req, const int* switches,
                                       int n_switches, mmda_misa_step_plan* out) {
  if (!m || !req || !out || B <= 0 || T <= 0 || (switches && n_switches != MMDA_MISA_STEP_SWITCHES)) return MMDA_EINVAL;
  static const float labels = 0.f; static const OptStep opt = {};      // stand for "given": plan_input tests the pointers only
  const StepRequest r{req->fused != 0, req->has_labels ? &labels : nullptr, req->has_opt_step ? &opt : nullptr, req->enc_cached != 0};
  StepSwitches sw;
  if (switches) memcpy(&sw, switches, sizeof(sw));
  const StepPlan P = plan_step(plan_input(m, r, B, T), sw);
  *out = mmda_misa_step_plan{P.fused, P.inf, P.enc_cut, P.enc_nostash, P.enc_cached, P.bfg, P.gm, P.kdg, P.tn_wgrad, P.want_b, P.want_c,
                             P.want_wT, P.wT_merge, P.skinny, P.row_fuse, P.ffn_fuse_fwd, P.ffn_fuse_bwd, P.seed_recon, P.seed_cls, P.fj_on,
                             P.fj_fwd, P.fj_device, P.zg_here, P.rec_hoisted, P.sort_early, P.embed_update, P.embed_deferred, P.embed_bg,
                             P.embed_bg_late, P.embed_bg_wgs, P.embed_bg_lds};
  return MMDA_OK;
}
namespace {
// abort words of the CURRENT exchange regions -> abort_sticky (synchronous device->host copies)
int harvest_abort(mmda_misa* m) {
  if (!m->ws || !m->xchg_ws || m->xchg_ws != m->ws) return MMDA_OK;
  for (int i = 0; i < 3; ++i) {
    if (m->lay.mod[i].xchg < 0) continue;
    unsigned w = 0;
    if (hipMemcpy(&w, m->ws + m->lay.mod[i].xchg, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return MMDA_ELAUNCH;
    if (w) m->abort_sticky = 1;
  }
  return MMDA_OK;
}
}  // namespace

extern "C" int mmda_misa_set_workspace_async(mmda_misa* m, float* ws, int64_t floats, int B, int T, void* stream) {
  if (!m || !ws || B <= 0 || T <= 0 || ((uintptr_t)ws & 15)) return MMDA_EINVAL;
  const Workspace w = carve(m->cfg, m->par, B, T);
  if (floats < w.floats) return MMDA_EINVAL;
  // The exchange regions keep their place and their contents while the buffer and B stay the same (a new T only): nothing to clear,
  // the flags there are monotonic epochs.  Otherwise they start from zero -- after the abort words of the old ones were looked at
  // (same buffer, new B: one synchronous read per region, rare; a NEW buffer: the caller reads mmda_misa_cluster_status first).
  const bool keep = m->xchg_ws == ws && m->xchg_B == B;
  if (!keep && m->xchg_ws == ws) { int rc = harvest_abort(m); if (rc) return rc; }
  m->rebind(w);
  m->ws = ws;
  hipStream_t s = (hipStream_t)stream;
  if (!keep) {
    for (int i = 0; i < 3; ++i)
      if (w.mod[i].xchg >= 0 && hipMemsetAsync(ws + w.mod[i].xchg, 0, sizeof(float) * w.mod[i].xchg_floats, s) != hipSuccess) return MMDA_ELAUNCH;
    m->xchg_ws = ws; m->xchg_B = B;
  }
  if (w.gpad_end > w.gpad_begin && hipMemsetAsync(ws + w.gpad_begin, 0, sizeof(float) * (w.gpad_end - w.gpad_begin), s) != hipSuccess)
    return MMDA_ELAUNCH;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_workspace(mmda_misa* m, float* ws, int64_t floats, int B, int T) {
  return mmda_misa_set_workspace_async(m, ws, floats, B, T, nullptr);       // the null stream: ordered against every blocking stream
}
extern "C" int64_t mmda_misa_tensor_offset(const mmda_misa* m, const char* name) {
  if (!m || !name || !m->ws) return -1;             // (no workspace bound yet: no name has an offset)
  return tensor_offset(m->lay, name);
}
extern "C" int mmda_misa_set_mode(mmda_misa* m, int mode) {
  if (!m || (mode != MMDA_F32 && mode != MMDA_BF16)) return MMDA_EINVAL;
  m->cfg.mode = mode;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_overlap(mmda_misa* m, int side_stream) {
  if (!m) return MMDA_EINVAL;
  m->use_side = side_stream ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_recurrence(mmda_misa* m, int resident_weights) {
  if (!m) return MMDA_EINVAL;
  m->use_cluster = resident_weights ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_gemm_operands(mmda_misa* m, int bf16_copies) {
  if (!m) return MMDA_EINVAL;
  m->use_bf16_gemm = bf16_copies ? 1 : 0;
  return MMDA_OK;
}
extern "C" int64_t mmda_misa_early_grad_floats(const mmda_misa* m) {
  return (m && m->early_valid) ? m->early_floats : 0;
}
extern "C" int mmda_misa_wait_early_grads(mmda_misa* m, void* stream) {
  if (!m || !m->early_valid || !m->ev_early) return MMDA_EINVAL;
  if (hipStreamWaitEvent((hipStream_t)stream, m->ev_early, 0) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_external_batch_losses(mmda_misa* m, int on) {
  if (!m) return MMDA_EINVAL;
  m->ext_batch_losses = on ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_inference(mmda_misa* m, int forward_only) {
  if (!m) return MMDA_EINVAL;
  m->inference = forward_only ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_cluster_status(const mmda_misa* m, int* aborted_host) {
  // reads the sticky abort words of the three exchange buffers (device->host copy: call it off the step path)
  if (!m || !m->ws || !aborted_host) return MMDA_EINVAL;
  *aborted_host = m->abort_sticky;          // seen in an exchange region that has since been cleared (B changed)
  if (m->jflags) {                          // a flag join timed out (see mmda_misa::jflags)
    unsigned w = 0;
    if (hipMemcpy(&w, m->jflags + 2, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return MMDA_ELAUNCH;
    if (w) *aborted_host |= 2;                 // (bit 1: a stream-to-stream flag wait, not a recurrence)
  }
  for (int i = 0; i < 3; ++i) {
    if (m->lay.mod[i].xchg < 0) continue;
    unsigned w = 0;
    if (hipMemcpy(&w, m->ws + m->lay.mod[i].xchg, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return MMDA_ELAUNCH;
    if (w) *aborted_host = 1;
  }
  return MMDA_OK;
}

// =============================================================================================== forward
namespace {
// K-major (transposed) fp32 copies of the fusion block's weights for its input-gradient GEMMs in the backward pass; issued on a side
// stream that the end of forward() joins
void weight_transpose_jobs(mmda_misa* m, std::vector<mmda_transpose_job>& tj) {
  const mmda_misa_config& c = m->cfg;
  const ParamTable& p = m->par; const Workspace& w = m->lay;
  const int hs_ = c.hidden, NC_ = 6 + c.ncls;
  auto T_ = [&](int64_t src, int rows, int cols, int64_t dst) { tj.push_back(mmda_transpose_job{PP(src), rows, cols, cols, WS(dst), rows}); };
  T_(p.head_w, NC_, 6 * hs_, w.head_wT); T_(p.l2_w, hs_, FFN, w.l2_wT); T_(p.l1_w, FFN, hs_, w.l1_wT);
  T_(p.out_w, hs_, hs_, w.out_wT); T_(p.in_w, 3 * hs_, hs_, w.in_wT); T_(p.sh_w, hs_, hs_, w.sh_wT);
  for (int i = 0; i < 3; ++i) {
    T_(p.rec_w + (int64_t)i * hs_ * hs_, hs_, hs_, w.rec_wT + (int64_t)i * hs_ * hs_);
    T_(p.priv_w + (int64_t)i * hs_ * hs_, hs_, hs_, w.priv_wT + (int64_t)i * hs_ * hs_);
    T_(p.mod[i].pw, hs_, 4 * p.mod[i].H, w.pwT[i]);
  }
  if (!c.use_cmd_sim) { T_(p.d1_w, hs_, hs_, w.d1_wT); T_(p.d2_w, 3, hs_, w.d2_wT); }
}
int weight_transposes(mmda_misa* m, void* ss) {
  std::vector<mmda_transpose_job> tj;
  weight_transpose_jobs(m, tj);
  const int rc = mmda_transpose_f32(tj.data(), (int)tj.size(), ss);
  m->wT_valid = rc ? 0 : 1;
  m->wT_pending = 0;
  return rc;
}

// bf16 operand copies that only the backward pass reads -- hseq of both layers (per direction for the tn weight-gradient GEMMs,
// transposed for the nt ones) and, nt only, the transposed layer-2 inputs: made on the side stream beside the fusion block.  <= 15 jobs.
int backward_only_jobs(mmda_misa* m, mmda_convert_job* cj) {
  const ParamTable& p = m->par; const Workspace& w = m->lay;
  const int R = w.B * w.T;
  int n = 0;
  for (int i = 0; i < 3; ++i) {
    const ModP& md = p.mod[i]; const ModW& mw = w.mod[i];
    for (int l = 0; l < 2; ++l) {
      const RnnP& r = md.rnn[l]; const RnnW& rw = mw.rnn[l];
      if (m->plan.tn_wgrad) {
        for (int d = 0; d < 2; ++d)
          cj[n++] = mmda_convert_job{WS(mw.hseq[l]) + d * md.H, 2 * md.H, R, md.H, nullptr, WS(rw.hbp[d]), r.ldH, nullptr, 0};
      } else {
        cj[n++] = mmda_convert_job{WS(mw.hseq[l]), 2 * md.H, R, 2 * md.H, nullptr, nullptr, 0, WS(rw.hbT), w.ldR};
      }
    }
    if (!m->plan.tn_wgrad) cj[n++] = mmda_convert_job{WS(mw.normed), 2 * md.H, R, 2 * md.H, nullptr, nullptr, 0, WS(mw.rnn[1].xbT), w.ldR};
  }
  return n;
}

// side stream, right after x6 = [private x3, shared x3] exists: clear the loss sums and the loss-seeded activation gradients,
// then DiffLoss and CMD with their gradients (they read x6 only), then the gradient bucket if train_step left that to forward()
int eager_side_losses(mmda_misa* m, void* stream) {
  const StepPlan& P = m->plan;
  if (!P.fused) return MMDA_OK;
  const mmda_misa_config& c = m->cfg; const Workspace& w = m->lay;
  const int B = w.B, hs = c.hidden;
  const int64_t BH = (int64_t)B * hs;
  void* ss = nullptr;
  int rc = side_fork(m, stream, &ss);
  // (large batches: the loss chain on the side stream is the longer one by far -- the weight transposes go to the main stream)
  if (!rc && m->wT_pending) rc = weight_transposes(m, B >= 128 ? stream : ss);
  // (the forward stretches on the main stream STORE the seeds they own: clearing those here would race with them)
  const int64_t zend = P.seed_cls ? w.zero_cls : P.seed_recon ? w.zero_recon : w.zero_end;
  // The gradient bucket (43 MB, 11 us) is cleared on the MAIN stream behind the fork: since the row-local stretches were fused the
  // side stream's loss chain (72 us at B=32), not the main stream's fusion block (55 us), is what the join at the end of forward() waits
  // for.  (Nothing on either stream touches the bucket before the backward pass; MMDA_ZERO_GRAD_SIDE=1: the old place.)
  // ... unless the main stream will not wait for this chain before the LayerNorm-1 stretch of the backward pass (flag join on the
  // device, small batches: see mmda_misa::jflags) -- the chain then has two launches of slack and the clear comes back here, in ONE
  // launch with the activation-gradient region, at the head of the chain.
  if (!rc && P.zg_here && m->zero_grad_pending) {
    rc = mmda_zero2(WS(w.zero_begin), zend - w.zero_begin, m->G, grad_floats(m), ss);
    m->zero_grad_pending = 0;
  } else if (!rc) {
    if (hipMemsetAsync(WS(w.zero_begin), 0, sizeof(float) * (zend - w.zero_begin), (hipStream_t)ss) != hipSuccess) rc = MMDA_ELAUNCH;
  }
  float* L = WS(w.losses);
  if (!rc) rc = mmda_loss_diff(WS(w.x6), BH, B, hs, c.diff_weight, L + 1, WS(w.d_x6), WS(w.diff_work), ss);
  // the chain's last launch sets the flag-join word itself where it can (single-workgroup CMD: no one-thread launch behind it)
  m->fj1_armed = (!rc && c.use_cmd_sim && P.fj_fwd && m->jflags && mmda_loss_cmd_sets_flag(B, hs)) ? 1 : 0;
  if (!rc && c.use_cmd_sim) {
    static const int sim_pairs[6] = {0, 1, 0, 2, 2, 1};      // what mmda_loss_cmd runs: (t,v), (t,a), (a,v), five moments, / 3
    rc = mmda_loss_cmd_pairs_tail(WS(w.x6 + 3 * BH), BH, 3, 3, sim_pairs, 5, B, hs, c.sim_weight, 1.0f / 3.0f, L + 2, WS(w.d_x6 + 3 * BH), ss,
                                  m->fj1_armed ? m->jflags + 0 : nullptr, m->jval[0] + 1);
  }
  if (!rc && m->zero_grad_pending) { rc = mmda_misa_zero_grad(m, stream); m->zero_grad_pending = 0; }
  m->eager_done = 1;
  return rc;
}
}  // namespace

namespace {
// feed-forward of the fusion transformer layer on block-scaled fp8 operands (models.py:160-161; torch's linear1 -> relu -> dropout ->
// linear2): x1 (6B, hs) -> f1 (6B, FFN) -> f2 (6B, hs).  Four launches: quantise {x1, W1, W2}, product 1 (+bias, relu, dropout),
// quantise f1, product 2 (+bias).  The f32 tensors f1 / f2 the backward pass reads are written as on the exact path.
int ffn_fp8(mmda_misa* m, float p_tf, uint64_t seed, void* stream) {
  const mmda_misa_config& c = m->cfg; const ParamTable& p = m->par; const Workspace& w = m->lay;
  const int hs = c.hidden, R6 = 6 * w.B;
  if ((hs % 128) != 0) return MMDA_EINVAL;               // K of product 1 must be whole 128-deep MFMA steps
  auto U8 = [&](int64_t off) { return reinterpret_cast<unsigned char*>(m->ws + off); };
  mmda_mx8_quant_job q[3] = {
      {m->ws + w.x1, hs, R6, hs, U8(w.x1q), U8(w.x1s)},
      {m->P + p.l1_w, hs, FFN, hs, U8(w.w1q), U8(w.w1s)},
      {m->P + p.l2_w, FFN, hs, FFN, U8(w.w2q), U8(w.w2s)}};
  int rc = mmda_mx8_quant(q, 3, stream);
  if (rc) return rc;
  mmda_mx8_args g = {};
  g.M = R6; g.N = FFN; g.K = hs; g.Aq = U8(w.x1q); g.As = U8(w.x1s); g.Bq = U8(w.w1q); g.Bs = U8(w.w1s);
  g.C = m->ws + w.f1; g.ldc = FFN; g.bias = m->P + p.l1_b; g.act = MMDA_ACT_RELU; g.drop_p = p_tf; g.drop_seed = seed; g.drop_site = SITE_FFN;
  rc = mmda_gemm_mx8(&g, stream);
  if (rc) return rc;
  mmda_mx8_quant_job qf = {m->ws + w.f1, FFN, R6, FFN, U8(w.f1q), U8(w.f1s)};
  rc = mmda_mx8_quant(&qf, 1, stream);
  if (rc) return rc;
  mmda_mx8_args h = {};
  h.M = R6; h.N = hs; h.K = FFN; h.Aq = U8(w.f1q); h.As = U8(w.f1s); h.Bq = U8(w.w2q); h.Bs = U8(w.w2s);
  h.C = m->ws + w.f2; h.ldc = hs; h.bias = m->P + p.l2_b;
  return mmda_gemm_mx8(&h, stream);
}
}  // namespace

extern "C" int mmda_misa_set_adam(mmda_misa* m, const mmda_adam_opts* opts, float clip_norm) {
  if (!m || !(clip_norm >= 0.f)) return MMDA_EINVAL;
  const mmda_adam_opts o = opts ? *opts : kAdamDefaults;
  if (!mmda_adam_opts_valid(&o)) return MMDA_EINVAL;
  // deferred table: the updates that stale rows are still to replay were made with the old betas and eps
  const bool moved = o.beta1 != m->adam.beta1 || o.beta2 != m->adam.beta2 || o.eps != m->adam.eps;
  if (moved && m->df_row_step && m->df_flushed != m->df_seq) return MMDA_EINVAL;
  m->adam = o; m->adam.scale_dev = nullptr;
  m->clip_norm = clip_norm;
  return MMDA_OK;
}

extern "C" int mmda_misa_set_cls_loss(mmda_misa* m, const mmda_cls_opts* opts) {
  if (!m || !mmda_cls_opts_valid(opts, m->cfg.ncls)) return MMDA_EINVAL;
  const int on = opts && !(opts->n_weights == 0 && opts->focal_gamma == 0.f);
  if (on && m->reg != REG_NONE) return MMDA_EINVAL;      // class weights and the focal exponent belong to the classifier
  m->cls_on = on;
  m->cls_opts = m->cls_on ? *opts : mmda_cls_opts{};
  return MMDA_OK;
}

extern "C" int mmda_misa_set_task(mmda_misa* m, int task, int loss_kind) {
  if (!m || (task != MMDA_TASK_EMOTION && task != MMDA_TASK_SENTIMENT)) return MMDA_EINVAL;
  if (task == MMDA_TASK_SENTIMENT) {
    if (loss_kind != MMDA_SENTI_L1 && loss_kind != MMDA_SENTI_MSE) return MMDA_EINVAL;
    // one output column; the confidence loss's target truth * pred is defined for labels in {0, 1}
    if (m->cfg.ncls != 1 || m->cfg.use_confidNet || m->cls_on) return MMDA_EINVAL;
  }
  m->reg = task == MMDA_TASK_SENTIMENT ? 1 + loss_kind : REG_NONE;
  return MMDA_OK;
}

extern "C" int mmda_misa_set_embed_update(mmda_misa* m, int mode) {
  if (!m) return MMDA_EINVAL;
  if (mode != EU_DENSE && mode != EU_SPARSE && mode != EU_FROZEN) return MMDA_EINVAL;
  if (mode != EU_DENSE) { m->df_row_step = nullptr; m->df_ring = nullptr; m->df_window = 0; }     // (the caller flushed first)
  m->embed_update = mode;
  m->eu.take();
  return MMDA_OK;
}

extern "C" int mmda_misa_set_embed_deferred(mmda_misa* m, int32_t* row_step, float* step_scalars, int window, void* stream) {
  if (!m) return MMDA_EINVAL;
  if (!row_step && !step_scalars) {                        // off: plain dense from the next step on (the caller flushed first)
    m->df_row_step = nullptr; m->df_ring = nullptr; m->df_window = 0; m->eu.take();
    return MMDA_OK;
  }
  if (!row_step || !step_scalars || window < 1 || m->embed_update != EU_DENSE) return MMDA_EINVAL;
  const int rc = mmda_embed_deferred_reset(row_step, m->cfg.vocab, stream);
  if (rc) return rc;
  m->df_row_step = row_step; m->df_ring = step_scalars; m->df_window = window; m->eu.take();
  m->df_seq = m->df_flushed = 0;
  return MMDA_OK;
}

extern "C" int mmda_misa_set_embed_background(mmda_misa* m, int on, int workgroups) {
  if (!m || (on != 0 && on != 1) || workgroups < 0 || workgroups > 4096) return MMDA_EINVAL;
  m->bg_on = on; m->bg_wgs = workgroups;
  return MMDA_OK;
}
extern "C" int mmda_misa_embed_background_active(const mmda_misa* m) { return m ? m->bg_active : MMDA_EINVAL; }

extern "C" int mmda_misa_embed_flush(mmda_misa* m, void* stream) {
  if (!m) return MMDA_EINVAL;
  if (!m->df_row_step) return MMDA_OK;                     // nothing is deferred
  if (!m->P || !m->M1 || !m->V1) return MMDA_EINVAL;
  if (m->df_flushed == m->df_seq) return MMDA_OK;          // no update since the last flush: nothing is stale, nothing is launched
  const int rc = mmda_embed_rows_flush(PP(m->par.embed), m->M1 + m->par.embed, m->V1 + m->par.embed, m->df_row_step, m->df_ring, m->df_window,
                                       m->cfg.d_t, m->cfg.vocab, m->adam.beta1, m->adam.beta2, m->adam.eps, m->df_seq, stream);
  if (!rc) m->df_flushed = m->df_seq;
  return rc;
}

namespace {
// update df_seq + 1 of the deferred table for the rows of one backward's id list, counted here and nowhere else
int deferred_apply(mmda_misa* m, const int64_t* ids, const unsigned* sorted, const int32_t* lengths, float lr, float beta1, float beta2,
                   float eps, float clip, float grad_scale, int step, bool catch_up, void* stream) {
  if (!m->df_row_step || !m->P || !m->M1 || !m->V1 || !m->ws || m->lay.T <= 0 || !ids) return MMDA_EINVAL;
  if (m->df_seq == INT32_MAX) return MMDA_EINVAL;
  const int seq = m->df_seq + 1;
  const int rc = mmda_embed_dense_adam_apply(PP(m->par.embed), m->M1 + m->par.embed, m->V1 + m->par.embed, m->df_row_step, m->df_ring, m->df_window, ids,
                                             sorted, m->lay.B * m->lay.T, m->cfg.d_t, WS(m->lay.mod[0].d_x), lengths, m->lay.B, m->cfg.vocab, lr, beta1,
                                             beta2, eps, clip, grad_scale, seq, step, catch_up, stream);
  if (rc) return rc;
  if (seq % m->df_window == 0) m->df_flushed = seq - 1;    // (that update flushed first)
  m->df_seq = seq;
  return MMDA_OK;
}
}  // namespace

extern "C" int mmda_misa_embed_deferred_step(mmda_misa* m, float lr, float beta1, float beta2, float eps, float clip, float grad_scale,
                                             int step, void* stream) {
  if (!m || !m->df_row_step || m->embed_update != EU_DENSE || !m->eu.on || step < 1) return MMDA_EINVAL;
  const PendingRows r = m->eu.take();
  // (another forward may have run since that backward: its rows are brought to the last update again, which costs one launch)
  return deferred_apply(m, r.ids, nullptr, r.lengths, lr, beta1, beta2, eps, clip, grad_scale, step, true, stream);
}

extern "C" int mmda_misa_set_fusion_fp8(mmda_misa* m, int on) {
  if (!m) return MMDA_EINVAL;
  if (on && (m->cfg.hidden % 128) != 0) return MMDA_EINVAL;
  m->fusion_fp8 = on ? 1 : 0;
  return MMDA_OK;
}

// ---- frozen parameters
extern "C" int mmda_misa_set_trainable(mmda_misa* m, const unsigned char* flags, int n_params) {
  if (!m || !flags || n_params != (int)m->par.params.size()) return MMDA_EINVAL;
  return apply_trainable(m, flags);
}
extern "C" int mmda_misa_trainable_info(const mmda_misa* m, mmda_run* runs, int capacity, int* n_runs, int64_t* trainable_floats,
                                        int* encoder_cut_on) {
  if (!m || capacity < 0 || (capacity > 0 && !runs)) return MMDA_EINVAL;
  // the table as its user sees it: runs that touch are one run, whichever section cut lies between them
  int n = 0; int64_t floats = 0, end = -1, items = 0;
  mmda_run last = {0, 0, 0};
  for (size_t i = 0; i + 1 < m->runs.size(); ++i) {
    const mmda_run& r = m->runs[i];
    floats += r.len;
    if (n > 0 && r.begin == end) {
      last.len += r.len;
    } else {
      if (n > 0) items += ((last.begin + last.len - 1) >> 2) - (last.begin >> 2) + 1;
      last = mmda_run{r.begin, r.len, items};
      ++n;
    }
    if (n <= capacity) runs[n - 1] = last;
    end = r.begin + r.len;
  }
  if (n_runs) *n_runs = n;
  if (trainable_floats) *trainable_floats = floats;
  if (encoder_cut_on) *encoder_cut_on = encoder_cut(m) ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_cut_forward(mmda_misa* m, int keep_stash) {
  if (!m) return MMDA_EINVAL;
  m->cut_keep_stash = keep_stash ? 1 : 0;
  return MMDA_OK;
}

namespace {
// One pass of the step in flight, as a sequence of stages: the GEMM context and what every stage reads -- the plan, the
// configuration, the batch shape and the dropout of the step.  Each stage sets rc and issues nothing once it is set.
struct Pass : Ctx {
  const StepPlan& P;
  const mmda_misa_config& c;
  const ParamTable& p; const Workspace& w;   // read-only views of the handle's two values: no stage moves an offset
  const int B, T, R, hs, NC, mode;
  static constexpr int fmode = MMDA_F32;     // the fusion block's GEMMs: exact path (see mmda_misa_forward)
  const int64_t BH; const float p_tf, p_cls; const uint64_t seed;
  // StepRequest::emo and ::opt of the pass.  opt, forward: its kind may run the background pass over the table (fwd_operands);
  // backward of a fused step: the optimizer step this pass may start (see bwd_encoder_layer)
  const float* emo; const OptStep* opt;
  Pass(mmda_misa* m_, void* s_, const float* emo_ = nullptr, const OptStep* opt_ = nullptr)
      : Ctx{m_, s_}, P(m_->plan), c(m_->cfg), p(m_->par), w(m_->lay), B(w.B), T(w.T), R(w.T * w.B), hs(c.hidden), NC(6 + c.ncls), mode(c.mode),
        BH((int64_t)B * hs), p_tf(m_->training ? c.fusion_dropout : 0.f), p_cls(m_->training ? c.dropout : 0.f), seed(m_->seed), emo(emo_), opt(opt_) {}
  mmda_ln_args proj_ln_fwd(int i), norm1_fwd(), norm2_fwd();             // LayerNorm arguments (builders below)
  mmda_ln_bwd_args proj_ln_bwd(int i), norm1_bwd(), norm2_bwd();
  // forward, in this order: operands, layers 1 and 2, the fusion block in one of two forms
  void fwd_operands(const int64_t* t_ids, const float* const* xin);
  void fwd_encoder_layer(int l, const float* const* xin, const int32_t* lengths);
  void fwd_fusion_skinny(), fwd_fusion_tiled();
  // backward, in this order: the fusion block's dX chain in one of three forms, its weight gradients, the side chain, layers 2 and 1
  void bwd_fusion_fused(), bwd_fusion_skinny(), bwd_fusion_tiled(), skinny_ffn_dx(bool wt), skinny_proj_dx(bool wt);
  void fusion_wgrads(), bwd_side_chain(bool pg_pending, const int64_t* t_ids, const int32_t* lengths);
  void bwd_encoder_layer(int l, const float* const* xin, const int64_t* t_ids, const int32_t* lengths);
  void bwd_text_rows(const int64_t* t_ids, const int32_t* lengths);
  const unsigned* take_sorted();
};

// LayerNorm arguments of the fusion block: the projections' (+ activation), norm1 and norm2 (residual and dropout ride along)
mmda_ln_args Pass::proj_ln_fwd(int i) {
  mmda_ln_args ln = {};
  ln.rows = B; ln.n = hs; ln.x = WS(w.z + i * BH); ln.gamma = PP(p.mod[i].plw); ln.beta = PP(p.mod[i].plb);
  ln.y = WS(w.orig + i * BH); ln.mean = WS(w.pmean + i * B); ln.rstd = WS(w.prstd + i * B); ln.act = c.act;
  ln.eps = 1e-5f; ln.actp = act_params(m, m->training, seed, SITE_RRELU + i, false);
  return ln;
}
mmda_ln_args Pass::norm1_fwd() {
  mmda_ln_args ln = {};
  ln.rows = 6 * B; ln.n = hs; ln.x = WS(w.x6); ln.res = WS(w.attn_out); ln.gamma = PP(p.n1_w); ln.beta = PP(p.n1_b);
  ln.y = WS(w.x1); ln.mean = WS(w.ln1_mean); ln.rstd = WS(w.ln1_rstd); ln.drop_p = p_tf; ln.drop_seed = seed;
  ln.drop_site = SITE_DROP1; ln.eps = 1e-5f;
  return ln;
}
mmda_ln_args Pass::norm2_fwd() {
  mmda_ln_args ln = {};
  ln.rows = 6 * B; ln.n = hs; ln.x = WS(w.x1); ln.res = WS(w.f2); ln.gamma = PP(p.n2_w); ln.beta = PP(p.n2_b);
  ln.y = WS(w.hfused); ln.mean = WS(w.ln2_mean); ln.rstd = WS(w.ln2_rstd); ln.drop_p = p_tf; ln.drop_seed = seed;
  ln.drop_site = SITE_DROP2; ln.permute_S = S6; ln.permute_B = B; ln.eps = 1e-5f;   // emits h = cat(h[0..5], dim=1)
  return ln;
}
mmda_ln_bwd_args Pass::proj_ln_bwd(int i) {
  mmda_ln_bwd_args l = {};
  l.rows = B; l.n = hs; l.dy = WS(w.d_orig + i * BH); l.x = WS(w.z + i * BH); l.gamma = PP(p.mod[i].plw);
  l.mean = WS(w.pmean + i * B); l.rstd = WS(w.prstd + i * B); l.d_x = WS(w.d_z + i * BH);
  l.dgamma = GG(p.mod[i].plw); l.dbeta = GG(p.mod[i].plb); l.act = c.act;
  l.actp = act_params(m, m->training, seed, SITE_RRELU + i, true);
  return l;
}
mmda_ln_bwd_args Pass::norm1_bwd() {
  mmda_ln_bwd_args l = {};
  l.rows = 6 * B; l.n = hs; l.dy = WS(w.d_x1); l.x = WS(w.x6); l.res = WS(w.attn_out); l.gamma = PP(p.n1_w);
  l.mean = WS(w.ln1_mean); l.rstd = WS(w.ln1_rstd); l.d_x = WS(w.d_x6); l.accumulate_dx = 1; l.d_res = WS(w.d_attn_out);
  l.dgamma = GG(p.n1_w); l.dbeta = GG(p.n1_b); l.drop_p = p_tf; l.drop_seed = seed; l.drop_site = SITE_DROP1;
  return l;
}
mmda_ln_bwd_args Pass::norm2_bwd() {
  mmda_ln_bwd_args l = {};
  l.rows = 6 * B; l.n = hs; l.dy = WS(w.d_hfused); l.x = WS(w.x1); l.res = WS(w.f2); l.gamma = PP(p.n2_w);
  l.mean = WS(w.ln2_mean); l.rstd = WS(w.ln2_rstd); l.d_x = WS(w.d_x1); l.d_res = WS(w.d_f2);
  l.dgamma = GG(p.n2_w); l.dbeta = GG(p.n2_b); l.drop_p = p_tf; l.drop_seed = seed; l.drop_site = SITE_DROP2;
  l.permute_S = S6; l.permute_B = B;
  return l;
}

// W_hh -> MFMA fragment order (weights changed since the last step), the bf16 operand copies or (fp32) the embedding rows
void Pass::fwd_operands(const int64_t* t_ids, const float* const* xin) {
  // bf16 mode: the input GEMMs read bf16 operand copies (K-major, 16-B rows): W_ih of both layers (plain for the forward,
  // transposed for dX) and the layer-1 inputs -- the text rows are gathered from the embedding matrix by the conversion itself
  // (models.py:201), so no fp32 copy of them is made.
  // The transposed copies, which only the backward pass reads, are made on the main stream with the forward ones.  (Making them on
  // the side stream beside the forward recurrences measured ~15 us slower: the fork's marker packet on the main stream and the L2
  // traffic beside the recurrences cost more than the smaller main-stream conversions save.)
  // the first conversions: W_ih of both layers and the layer-1 inputs, plain and (`transposed`) K-major
  auto first_jobs = [&](bool transposed, mmda_convert_job* cj) -> int {
    int n = 0;
    for (int i = 0; i < 3; ++i) {
      for (int l = 0; l < 2; ++l) {
        const RnnP& r = p.mod[i].rnn[l]; const RnnW& rw = w.mod[i].rnn[l];
        cj[n++] = mmda_convert_job{rW_ih(m, i, l), r.D, 8 * r.H, r.D, nullptr, WS(rw.wb), r.ldD,
                                   transposed ? WS(rw.wbT) : nullptr, transposed ? r.ldG : 0, P.gm ? r.H : 0};
      }
      const RnnP& r0 = p.mod[i].rnn[0]; const RnnW& rw0 = w.mod[i].rnn[0];
      const float* src = i == 0 ? PP(p.embed) : xin[i];
      const bool xt = transposed && !P.tn_wgrad;         // layer-1 inputs transposed: only the nt form of layer 1's dW_ih reads them
      cj[n++] = mmda_convert_job{src, r0.D, R, r0.D, i == 0 ? t_ids : nullptr, WS(rw0.xb), r0.ldD, xt ? WS(rw0.xbT) : nullptr, xt ? w.ldR : 0};
    }
    return n;
  };
  // bf16 operand copies in use: the twelve packings and the first conversions go out as ONE launch on the main stream
  // (mmda_lstm_pack_whh_and_convert) -- no fork, no cross-stream wait in front of the first recurrent kernel (each costs the main stream
  // 4 - 14 us).  The K-major copies of the fusion block's weights, which only the backward pass reads, then ride on the first fork that
  // happens anyway (wT_pending).  (Merged measured equal to round 1's form -- packing on the side stream, joined by an event -- which
  // the fp32 mode keeps.)
  m->wT_pending = 0;
  int Hs[12]; const float* Wp[12]; void* Fp[12]; void* Bp[12]; void* Cp[12];
  int k = 0;
  for (int i = 0; i < 3; ++i)
    for (int l = 0; l < 2; ++l)
      for (int d = 0; d < 2; ++d, ++k) {
        const RnnP& r = p.mod[i].rnn[l]; const RnnW& rw = w.mod[i].rnn[l];
        Hs[k] = r.H; Wp[k] = rW_hh(m, i, l, d); Fp[k] = WS(rw.pack_f[d]); Bp[k] = P.want_b ? WS(rw.pack_b[d]) : nullptr; Cp[k] = WS(rw.pack_c[d]);
      }
  m->wT_valid = 0;
  if (P.bfg) {
    mmda_convert_job cj[9];
    const int nj = first_jobs(!P.enc_nostash, cj);
    // ... and the K-major copies of the fusion block's weights (backward pass) in the same launch: 6 MB of traffic that cost a
    // launch of its own 7 - 9 us at the head of the loss chain (side stream, the longer of the two chains beside the fusion block)
    // or, at B >= 128, 15 us with its gap on the main stream.  MMDA_WT_MERGE=0: on the first fork as before.
    std::vector<mmda_transpose_job> tj;
    if (P.wT_merge) weight_transpose_jobs(m, tj);
    if (tj.size() > 20) tj.clear();
    RowStamp st;
    if (P.embed_bg) rc = bg_begin(m, t_ids, R, s, &st);
    if (!rc) rc = mmda_lstm_pack_convert_transpose_stamped(12, Hs, Wp, Fp, Bp, P.want_c ? Cp : nullptr, cj, nj, tj.data(), (int)tj.size(),
                                                           P.embed_bg ? &st : nullptr, s);
    m->wT_pending = (P.want_wT && tj.empty()) ? 1 : 0;
    if (!tj.empty()) m->wT_valid = rc ? 0 : 1;
  } else {
    void* ss = nullptr;
    rc = side_fork(m, s, &ss);
    if (!rc) rc = mmda_lstm_pack_whh_multi(mode, 12, Hs, Wp, Fp, Bp, P.want_c ? Cp : nullptr, ss);
    // the first recurrent kernel waits for the packing only, not for the transposes issued behind it
    if (!rc && ss != s && hipEventRecord(m->ev_pack, (hipStream_t)ss) != hipSuccess) rc = MMDA_ELAUNCH;
    if (!rc && P.want_wT) rc = weight_transposes(m, ss);
    // embedding rows (models.py:201)
    RowStamp st;
    if (!rc && P.embed_bg) rc = bg_begin(m, t_ids, R, s, &st);
    if (!rc) rc = mmda_embed_gather_stamped(PP(p.embed), t_ids, R, m->cfg.d_t, WS(w.mod[0].x), P.embed_bg ? &st : nullptr, s);
  }
  // the background pass over the table rows this batch does not index: forked here, behind the launch that stamped the others
  if (!rc && P.embed_bg && !P.embed_bg_late) rc = bg_launch(m, opt, s);
}

// encoder layer l: input GEMM and recurrence of the three modalities; then layer 1's LayerNorm, or layer 2's fork beside the fusion block
void Pass::fwd_encoder_layer(int l, const float* const* xin, const int32_t* lengths) {
  mmda_lstm_desc desc[3];
  mmda_gemm_bf16_args bg[3];
  group_begin(*this);
  for (int i = 0; i < 3; ++i) {
    const RnnP& r = p.mod[i].rnn[l]; const ModW& mw = w.mod[i]; const RnnW& rw = mw.rnn[l];
    const float* in = l == 0 ? xin[i] : WS(mw.normed);
    // time-batched input-to-hidden GEMM for both directions: (R, D) x (8H, D)^T + b_ih + b_hh
    if (P.bfg) {
      bg[i] = mmda_gemm_bf16_args{};
      bg[i].M = R; bg[i].N = 8 * r.H; bg[i].K = r.D; bg[i].A = WS(rw.xb); bg[i].lda = r.ldD; bg[i].B = WS(rw.wb); bg[i].ldb = r.ldD;
      bg[i].C = WS(mw.gates[l]); bg[i].ldc = 8 * r.H; bg[i].bias = rB_ih(m, i, l); bg[i].bias2 = rB_hh(m, i, l);
      bg[i].perm_n_H = P.gm ? r.H : 0;
    } else {
      gemm(*this, mode, 0, 1, R, 8 * r.H, r.D, in, r.D, rW_ih(m, i, l), r.D, WS(mw.gates[l]), 8 * r.H, rB_ih(m, i, l), rB_hh(m, i, l));
    }
    desc[i] = lstm_desc(m, i, l, false, P.gm, false);
    desc[i].forward_only = P.enc_nostash;
  }
  if (P.bfg && !rc) rc = mmda_gemm_bf16_grouped(bg, 3, s);
  m->epoch += (unsigned)T + 2u;
  group_end(*this);
  if (!rc && l == 0 && m->side_pending && m->use_side) {   // packed W_hh ready (the side stream carries on with its transposes)
    if (hipStreamWaitEvent((hipStream_t)s, m->ev_pack, 0) != hipSuccess) rc = MMDA_ELAUNCH;
  }
  if (rc) return;
  ev_rec(m, m->ev_fwd, l, 0, s);
  rc = mmda_lstm_fwd(mode, 3, desc, B, T, lengths, s);
  ev_rec(m, m->ev_fwd, l, 1, s);
  if (rc) return;
  if (l == 0 && P.embed_bg && P.embed_bg_late) { rc = bg_launch(m, opt, s); if (rc) return; }     // (MMDA_EMBED_BG_LATE=1: the later fork)
  if (l == 0) {
    mmda_ln_args ln[3];
    for (int i = 0; i < 3; ++i) {
      const ModP& md = p.mod[i]; const ModW& mw = w.mod[i];
      ln[i] = mmda_ln_args{};
      ln[i].rows = R; ln[i].n = 2 * md.H; ln[i].x = WS(mw.hseq[0]); ln[i].gamma = PP(md.ln_w); ln[i].beta = PP(md.ln_b);
      ln[i].y = WS(mw.normed); ln[i].mean = WS(mw.ln_mean); ln[i].rstd = WS(mw.ln_rstd); ln[i].eps = 1e-5f;
    }
    // (bf16 GEMMs: the LayerNorm also writes its output as the bf16 operand copy layer 2's input GEMM reads; the copies that only
    //  the backward pass needs -- hseq, transposed inputs -- are made later on the side stream: backward_only_jobs)
    if (P.bfg)
      for (int i = 0; i < 3; ++i) { ln[i].y_bf16 = WS(w.mod[i].rnn[1].xb); ln[i].ld_bf16 = p.mod[i].rnn[1].ldD; }
    // ... and ONLY as that copy where nothing reads the fp32 output: a pass whose encoders keep no stash, or a training step whose
    // layer-2 weight gradients take the tn form (they read the bf16 copy; the nt form converts the fp32 output into a transposed copy)
    if (P.bfg && (P.enc_nostash || P.tn_wgrad))
      for (int i = 0; i < 3; ++i) ln[i].y = nullptr;
    rc = mmda_layernorm_fwd_multi(ln, 3, s);
  } else if (!P.fused && ((P.bfg && !P.enc_nostash) || m->zero_grad_pending || m->wT_pending)) {
    // side stream, beside the fusion block: the gradient bucket is cleared (train_step) and hseq^T of layer 2 is made for its
    // dW_hh.  Joined at the end of forward(), so everything the backward pass issues on either stream is ordered behind both.
    void* ss = nullptr;
    rc = side_fork(m, s, &ss);
    if (!rc && m->wT_pending) rc = weight_transposes(m, ss);
    if (!rc && m->zero_grad_pending && !P.fused) { rc = mmda_misa_zero_grad(m, ss); m->zero_grad_pending = 0; }
  }
}

// shared_private (models.py:265-279) onwards, few rows: row-skinny GEMMs, independent ones grouped per launch (12 launches for the
// whole block) -- or the fused row-local stretches (P.row_fuse)
void Pass::fwd_fusion_skinny() {
  mmda_skinny_args g[8];
  mmda_ln_args ln[3];
  for (int i = 0; i < 3; ++i) {
    const ModP& md = p.mod[i]; const ModW& mw = w.mod[i];
    g[i] = sk_nt(B, hs, 4 * md.H, WS(mw.utt), 4 * md.H, PP(md.pw), PP(md.pb), WS(w.z + i * BH), hs);
    ln[i] = proj_ln_fwd(i);
  }
  sk_launch(*this, g, 3);
  if (!rc) rc = mmda_layernorm_fwd_multi(ln, 3, s);
  // private x3 and shared (one weight over the stacked 3B rows), sigmoid epilogue
  for (int i = 0; i < 3; ++i)
    g[i] = sk_nt(B, hs, hs, WS(w.orig + i * BH), hs, PP(p.priv_w + (int64_t)i * hs * hs), PP(p.priv_b + i * hs), WS(w.x6 + i * BH), hs,
                 MMDA_ACT_SIGMOID);
  g[3] = sk_nt(3 * B, hs, hs, WS(w.orig), hs, PP(p.sh_w), PP(p.sh_b), WS(w.x6 + 3 * BH), hs, MMDA_ACT_SIGMOID);
  sk_launch(*this, g, 4);
  if (!rc) rc = eager_side_losses(m, s);
  const mmda_ln_args l1 = norm1_fwd();
  if (P.row_fuse) {
    if (!rc) {
      FusedFwdA f = {};
      // one sample per workgroup in every stretch (two measured B=32 0.722 ms against 0.712; B=256 equal)
      f.B = B; f.hs = hs; f.nhead = NHEAD; f.nb = 1; f.x6 = WS(w.x6);
      f.rec_w = PP(p.rec_w); f.rec_b = PP(p.rec_b); f.recon = WS(w.recon);
      f.in_w = PP(p.in_w); f.in_b = PP(p.in_b); f.qkv = WS(w.qkv);
      f.ctx = WS(w.ctx); f.probs = WS(w.probs); f.p_tf = p_tf; f.seed = seed; f.site_attn = SITE_ATTN;
      f.out_w = PP(p.out_w); f.out_b = PP(p.out_b); f.attn_out = WS(w.attn_out); f.ln1 = l1;
      if (P.seed_recon) {
        f.orig = WS(w.orig); f.d_recon = WS(w.d_recon); f.d_orig = WS(w.d_orig);
        f.recon_inv_n = 1.0f / (float)(3 * BH); f.recon_scale = c.recon_weight;
      }
      rc = mmda_fused_fwd_a(&f, s);
    }
  } else {
    // reconstruct from private + shared (models.py:254-262), the q/k/v projection of the six tokens (models.py:243) and the
    // discriminator's first layer all read x6 only
    int n = 0;
    for (int i = 0; i < 3; ++i) {
      g[n] = sk_nt(B, hs, hs, WS(w.x6 + i * BH), hs, PP(p.rec_w + (int64_t)i * hs * hs), PP(p.rec_b + i * hs), WS(w.recon + i * BH), hs);
      g[n++].A2 = WS(w.x6 + (3 + i) * BH);
    }
    g[n++] = sk_nt(6 * B, 3 * hs, hs, WS(w.x6), hs, PP(p.in_w), PP(p.in_b), WS(w.qkv), 3 * hs);
    if (!c.use_cmd_sim) g[n++] = sk_nt(3 * B, hs, hs, WS(w.x6 + 3 * BH), hs, PP(p.d1_w), PP(p.d1_b), WS(w.dom_z), hs);
    sk_launch(*this, g, n);
    if (!c.use_cmd_sim && !rc) {
      const mmda_act_params ap = act_params(m, m->training, seed, SITE_RRELU_DISC, false);
      rc = mmda_act_dropout_fwd_p(WS(w.dom_z), WS(w.dom_h), 3 * BH, c.act, &ap, p_cls, seed, SITE_DISC, s);
    }
    if (!rc) rc = mmda_attn_fwd(WS(w.qkv), S6, B, hs, NHEAD, WS(w.ctx), WS(w.probs), p_tf, seed, SITE_ATTN, s);
    n = 0;
    g[n++] = sk_nt(6 * B, hs, hs, WS(w.ctx), hs, PP(p.out_w), PP(p.out_b), WS(w.attn_out), hs);
    if (!c.use_cmd_sim) g[n++] = sk_nt(3 * B, 3, hs, WS(w.dom_h), hs, PP(p.d2_w), PP(p.d2_b), WS(w.dom), 3);
    sk_launch(*this, g, n);
    if (!rc) rc = mmda_layernorm_fwd(&l1, s);
  }
  // feed-forward pair: one launch split over the hidden units (fused_rows.hip), its partial products summed by the stretch behind it
  if (m->fusion_fp8) {
    if (!rc) rc = ffn_fp8(m, p_tf, seed, s);
  } else if (P.ffn_fuse_fwd) {
    if (!rc) {
      FusedFfnFwd f = {};
      f.M = 6 * B; f.hs = hs; f.F = FFN; f.S = 32; f.x1 = WS(w.x1); f.w1 = PP(p.l1_w); f.b1 = PP(p.l1_b); f.f1 = WS(w.f1);
      f.p = p_tf; f.seed = seed; f.site = SITE_FFN; f.w2 = PP(p.l2_w); f.parts = WS(w.ffn_parts);
      rc = mmda_fused_ffn_fwd(&f, s);
    }
  } else {
    g[0] = sk_nt(6 * B, FFN, hs, WS(w.x1), hs, PP(p.l1_w), PP(p.l1_b), WS(w.f1), FFN, MMDA_ACT_RELU);
    g[0].drop_p = p_tf; g[0].drop_seed = seed; g[0].drop_site = SITE_FFN;
    sk_launch(*this, g, 1);
    g[0] = sk_nt(6 * B, hs, FFN, WS(w.f1), FFN, PP(p.l2_w), PP(p.l2_b), WS(w.f2), hs);
    sk_launch(*this, g, 1);
  }
  const mmda_ln_args l2 = norm2_fwd();
  if (P.row_fuse) {
    if (!rc) {
      FusedFwdC f = {};
      f.B = B; f.hs = hs; f.ncls = c.ncls; f.nb = 1; f.ln2 = l2;
      if (P.ffn_fuse_fwd) { f.ffn_parts = WS(w.ffn_parts); f.n_parts = FFN / 32; f.b2 = PP(p.l2_b); f.f2 = WS(w.f2); }
      f.hfused = WS(w.hfused); f.head_w = PP(p.head_w); f.head_b = PP(p.head_b); f.logits = WS(w.logits);
      f.threshold = c.threshold; f.tcp = WS(w.tcp); f.scores = WS(w.scores); f.labels = WS(w.labels);
      f.p_cls = p_cls; f.seed = seed; f.site_cls = SITE_CLS; f.reg = m->reg;
      if (P.seed_cls) { f.emo = emo; f.d_scores = WS(w.d_scores); f.cls = cls_term_of(m->cls()); }
      rc = mmda_fused_fwd_c(&f, s);
    }
  } else {
    if (!rc) rc = mmda_layernorm_fwd(&l2, s);
    g[0] = sk_nt(B, NC, 6 * hs, WS(w.hfused), 6 * hs, PP(p.head_w), PP(p.head_b), WS(w.logits), NC);
    sk_launch(*this, g, 1);
    if (!rc)
      rc = mmda_heads_fwd_task(WS(w.logits), B, c.ncls, c.threshold, WS(w.tcp), WS(w.scores), WS(w.labels), p_cls, seed, SITE_CLS,
                                 m->reg != REG_NONE, s);
  }
}

// the same, many rows: the tiled generic kernel
void Pass::fwd_fusion_tiled() {
  for (int i = 0; i < 3 && !rc; ++i) {
    const ModP& md = p.mod[i]; const ModW& mw = w.mod[i];
    lin_fwd(*this, fmode, B, hs, 4 * md.H, WS(mw.utt), PP(md.pw), PP(md.pb), WS(w.z + i * BH));
    if (rc) break;
    const mmda_ln_args ln = proj_ln_fwd(i);
    rc = mmda_layernorm_fwd(&ln, s);
  }
  // private (three weights, batched) and shared (one weight over the stacked 3B rows), sigmoid epilogue
  gemm(*this, fmode, 0, 1, B, hs, hs, WS(w.orig), hs, PP(p.priv_w), hs, WS(w.x6), hs, PP(p.priv_b), nullptr, 0, MMDA_ACT_SIGMOID, 3,
       BH, (int64_t)hs * hs, BH, hs);
  gemm(*this, fmode, 0, 1, 3 * B, hs, hs, WS(w.orig), hs, PP(p.sh_w), hs, WS(w.x6 + 3 * BH), hs, PP(p.sh_b), nullptr, 0,
       MMDA_ACT_SIGMOID);
  if (!rc) rc = eager_side_losses(m, s);
  // reconstruct (models.py:254-262)
  if (!rc) rc = mmda_add(WS(w.x6), WS(w.x6 + 3 * BH), WS(w.rsum), 3 * BH, s);
  gemm(*this, fmode, 0, 1, B, hs, hs, WS(w.rsum), hs, PP(p.rec_w), hs, WS(w.recon), hs, PP(p.rec_b), nullptr, 0, 0, 3, BH,
       (int64_t)hs * hs, BH, hs);
  // adversarial discriminator behind the gradient-reversal layer (models.py:219-227); identity in forward
  if (!c.use_cmd_sim) {
    lin_fwd(*this, fmode, 3 * B, hs, hs, WS(w.x6 + 3 * BH), PP(p.d1_w), PP(p.d1_b), WS(w.dom_z));
    if (!rc) {
      const mmda_act_params ap = act_params(m, m->training, seed, SITE_RRELU_DISC, false);
      rc = mmda_act_dropout_fwd_p(WS(w.dom_z), WS(w.dom_h), 3 * BH, c.act, &ap, p_cls, seed, SITE_DISC, s);
    }
    lin_fwd(*this, fmode, 3 * B, 3, hs, WS(w.dom_h), PP(p.d2_w), PP(p.d2_b), WS(w.dom));
  }
  // 1-layer transformer fusion over the six tokens (models.py:243-245; torch post-norm encoder layer)
  lin_fwd(*this, fmode, 6 * B, 3 * hs, hs, WS(w.x6), PP(p.in_w), PP(p.in_b), WS(w.qkv));
  if (!rc) rc = mmda_attn_fwd(WS(w.qkv), S6, B, hs, NHEAD, WS(w.ctx), WS(w.probs), p_tf, seed, SITE_ATTN, s);
  lin_fwd(*this, fmode, 6 * B, hs, hs, WS(w.ctx), PP(p.out_w), PP(p.out_b), WS(w.attn_out));
  const mmda_ln_args l1 = norm1_fwd(), l2 = norm2_fwd();
  if (!rc) rc = mmda_layernorm_fwd(&l1, s);
  if (m->fusion_fp8) {
    if (!rc) rc = ffn_fp8(m, p_tf, seed, s);
  } else {
    mmda_gemm_args e = {};
    e.drop_p = p_tf; e.drop_seed = seed; e.drop_site = SITE_FFN;
    gemm(*this, fmode, 0, 1, 6 * B, FFN, hs, WS(w.x1), hs, PP(p.l1_w), hs, WS(w.f1), FFN, PP(p.l1_b), nullptr, 0, MMDA_ACT_RELU, 1, 0,
         0, 0, 0, &e);
    lin_fwd(*this, fmode, 6 * B, hs, FFN, WS(w.f1), PP(p.l2_w), PP(p.l2_b), WS(w.f2));
  }
  if (!rc) rc = mmda_layernorm_fwd(&l2, s);
  // heads (models.py:247-249)
  lin_fwd(*this, fmode, B, NC, 6 * hs, WS(w.hfused), PP(p.head_w), PP(p.head_b), WS(w.logits));
  if (!rc)
    rc = mmda_heads_fwd_task(WS(w.logits), B, c.ncls, c.threshold, WS(w.tcp), WS(w.scores), WS(w.labels), p_cls, seed, SITE_CLS,
                               m->reg != REG_NONE, s);
}
}  // namespace

namespace {
// A forward pass from the projections on -- utt_t / utt_v / utt_a are in the workspace, from the encoders or from the encoder cache --
// and its tail: the K-major weight copies nobody has made yet, then the side stream's chain joined, on the device by the backward
// pass's stretch A (flag join) or by an event here.
int forward_from_projections(Pass& x, void* stream) {
  mmda_misa* m = x.m;
  if (m->plan.skinny) x.fwd_fusion_skinny();
  else x.fwd_fusion_tiled();
  if (!x.rc && m->wT_pending) {                // no fork came by (the eager losses are off and nothing else was pending)
    void* ss = nullptr;
    x.rc = side_fork(m, stream, &ss);
    if (!x.rc) x.rc = weight_transposes(m, ss);
  }
  if (!x.rc && m->plan.fj_fwd && m->side_pending && m->jflags) {
    x.rc = side_flag_signal(m, 0, m->fj1_armed != 0);      // (see mmda_misa::jflags: fused_bwd_a_kernel waits for the loss chain)
    m->fj1 = x.rc ? 0 : 1; m->fj1_armed = 0;
    return x.rc;
  }
  if (m->fj1_armed) return MMDA_ELAUNCH;       // (the CMD launch was armed on the same condition: cannot happen)
  if (!x.rc) x.rc = side_join(m, stream);      // (the side stream finished long ago: this only orders later work behind it)
  return x.rc;
}

bool encoded_batch_ok(const mmda_misa* m, const mmda_encoded_batch* eb) {
  return eb && eb->tab_t && eb->tab_v && eb->tab_a && eb->rows && eb->B > 0 && eb->B == m->lay.B;
}

// The forward pass of a step that starts behind the encoders: the plan, ONE gather of the batch's cached rows into utt_t / utt_v /
// utt_a (and of its labels into emo_out), then the fusion block as ever.  Skipped with the encoders: the GRU parameter padding, the
// deferred table's catch-up, fwd_operands, both encoder layers and the cluster epochs they advance (no recurrence is launched).  What
// fwd_operands does for the REST of the step is kept: the K-major fusion-weight copies take the wT_pending route -- the first fork, or
// the tail above -- in both precisions, since the conversion launch they ride in the bf16 mode does not exist here.
int forward_encoded(mmda_misa* m, const StepRequest& req, const mmda_encoded_batch* eb, float* emo_out, int training, uint64_t seed,
                    void* stream) {
  m->training = training; m->seed = seed;
  m->plan = plan_step(plan_input(m, req, m->lay.B, m->lay.T), step_switches());
  Pass x(m, stream, req.emo, req.opt);
  m->wT_valid = 0;
  m->wT_pending = m->plan.want_wT ? 1 : 0;
  x.rc = mmda_encoded_gather(eb->tab_t, eb->tab_v, eb->tab_a, 4 * m->par.mod[0].H, 4 * m->par.mod[1].H, 4 * m->par.mod[2].H,
                             emo_out ? eb->tab_emo : nullptr, m->cfg.ncls, eb->rows, m->lay.B, WS(m->lay.mod[0].utt), WS(m->lay.mod[1].utt),
                             WS(m->lay.mod[2].utt), emo_out, stream);
  if (x.rc) return x.rc;
  return forward_from_projections(x, stream);
}

// The forward pass from a batch, as `req` asks for it (mmda_misa_forward: StepRequest{}; train_step: its own)
int forward_pass(mmda_misa* m, const StepRequest& req, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                 int training, uint64_t seed, void* stream) {
  if (check_ready(m) || !t_ids || !v || !a || !lengths) return MMDA_EINVAL;
  // The fusion block (projections, private/shared/recon, transformer layer, heads) is 2 % of the FLOPs and feeds the
  // batch-statistic losses: it always runs on the exact f32 MFMA path.  `mode` (bf16) covers the LSTM GEMMs + recurrences.
  m->training = training; m->seed = seed;
  m->plan = plan_step(plan_input(m, req, m->lay.B, m->lay.T), step_switches());
  Pass x(m, stream, req.emo, req.opt);
  if (is_gru(m)) {          // GRU parameters -> four-slot layout (everything below reads the padded copies)
    mmda_gru_pad_job gj[MMDA_GRU_PAD_MAX];
    int n = gru_jobs(m, m->P, false, gj);
    x.rc = mmda_gru_pad_params(gj, n, stream);
    if (x.rc) return x.rc;
  }
  // deferred table update: the rows this batch gathers take the steps they missed first, so the gather reads what dense Adam left
  if (m->plan.embed_deferred) {
    if (!m->M1 || !m->V1) return MMDA_EINVAL;
    x.rc = mmda_embed_rows_catch_up(PP(m->par.embed), m->M1 + m->par.embed, m->V1 + m->par.embed, m->df_row_step, m->df_ring, m->df_window, t_ids,
                                    m->lay.B * m->lay.T, m->cfg.d_t, lengths, m->lay.B, m->cfg.vocab, m->adam.beta1, m->adam.beta2, m->adam.eps, m->df_seq, stream);
    if (x.rc) return x.rc;
  }
  const float* xin[3] = {WS(m->lay.mod[0].x), v, a};
  x.fwd_operands(t_ids, xin);
  for (int l = 0; l < 2 && !x.rc; ++l) x.fwd_encoder_layer(l, xin, lengths);
  if (x.rc) return x.rc;
  if (!m->ev.empty()) { if (m->ev_seen_f % m->ev_stride == 0) m->ev_fwd++; m->ev_seen_f++; }      // (the recurrent launches' timing)
  return forward_from_projections(x, stream);
}
}  // namespace

extern "C" int mmda_misa_forward_encoded(mmda_misa* m, const mmda_encoded_batch* eb, int training, uint64_t seed, void* stream) {
  if (check_ready(m) || !encoded_batch_ok(m, eb)) return MMDA_EINVAL;
  // a training forward: utt would need a gradient path that nobody computes
  if (!m->inference && !encoder_cut(m)) return MMDA_EINVAL;
  return forward_encoded(m, StepRequest{false, nullptr, nullptr, true}, eb, nullptr, training, seed, stream);
}

extern "C" int mmda_misa_forward(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                                 int training, uint64_t seed, void* stream) {
  return forward_pass(m, StepRequest{}, t_ids, v, a, lengths, training, seed, stream);
}

// =============================================================================================== losses
extern "C" int mmda_misa_zero_act_grads(mmda_misa* m, void* stream) {
  if (check_ready(m)) return MMDA_EINVAL;
  if (hipMemsetAsync(WS(m->lay.zero_begin), 0, sizeof(float) * (m->lay.zero_end - m->lay.zero_begin), (hipStream_t)stream) != hipSuccess)
    return MMDA_ELAUNCH;
  return MMDA_OK;
}

extern "C" int mmda_misa_losses(mmda_misa* m, const float* emo, int with_grads, void* stream) {
  if (check_ready(m) || !emo) return MMDA_EINVAL;
  const mmda_misa_config& c = m->cfg; const Workspace& w = m->lay;
  const int B = w.B, hs = c.hidden;
  const int64_t BH = (int64_t)B * hs;
  hipStream_t s = (hipStream_t)stream;
  int rc = MMDA_OK;
  float* L = WS(w.losses);
  const bool ext = m->ext_batch_losses && with_grads && c.use_cmd_sim;      // the caller did (see mmda_misa::ext_batch_losses)
  const bool eager = (m->eager_done || ext) && with_grads;        // forward() already cleared the region and ran diff (+ CMD) on the side stream
  // seeds the forward stretches stored already: the plan's, while this call takes up that forward pass's chain (eager_done)
  const bool s_recon = m->eager_done && with_grads && m->plan.seed_recon, s_cls = m->eager_done && with_grads && m->plan.seed_cls;
  m->eager_done = 0;
  if (eager) {
    rc = side_join(m, stream);                           // (forward() joined already; kept for callers that split the calls)
    if (rc) return rc;
  } else {
    if (with_grads) { rc = mmda_misa_zero_act_grads(m, stream); if (rc) return rc; }      // covers the loss sums too
    else if (hipMemsetAsync(WS(w.losses), 0, sizeof(float) * 8, s) != hipSuccess) return MMDA_ELAUNCH;
    rc = mmda_loss_diff(WS(w.x6), BH, B, hs, c.diff_weight, L + 1, with_grads ? WS(w.d_x6) : nullptr, WS(w.diff_work), stream);
    if (rc) return rc;
  }
  if (c.use_cmd_sim) {
    if (!eager) rc = mmda_loss_cmd(WS(w.x6 + 3 * BH), BH, B, hs, c.sim_weight, L + 2, with_grads ? WS(w.d_x6 + 3 * BH) : nullptr, stream);
  } else {
    rc = mmda_loss_domain(WS(w.dom), B, c.sim_weight, L + 2, with_grads ? WS(w.d_dom) : nullptr, stream);
  }
  if (rc) return rc;
  // cls, conf (computed every step like solver.py:168; it only seeds gradients with use_confidNet, solver.py:180-181), recon and
  // the weighted total in one launch
  if (s_recon && s_cls && c.use_cmd_sim) {
    // no gradient left to seed: the launch only computes loss values -- issued by backward() on the side stream (train_step calls it next)
    m->misc_deferred = emo;
    return MMDA_OK;
  }
  return mmda_loss_misc_reg(WS(w.scores), WS(w.tcp), emo, B, c.ncls, (with_grads && !s_cls) ? WS(w.d_scores) : nullptr,
                            (with_grads && !s_cls) ? WS(w.d_tcp) : nullptr, c.ncls == 6 && !ext, with_grads && c.use_confidNet && !ext,
                            c.conf_weight, WS(w.recon), WS(w.orig), 3 * BH, c.recon_weight, (with_grads && !s_recon) ? WS(w.d_recon) : nullptr,
                            (with_grads && !s_recon) ? WS(w.d_orig) : nullptr, L, c.diff_weight, c.sim_weight, c.recon_weight, c.conf_weight,
                            c.use_confidNet, m->cls(), m->reg, stream);
}

// =============================================================================================== backward
extern "C" int mmda_misa_zero_grad(mmda_misa* m, void* stream) {
  if (!m || !m->G) return MMDA_EINVAL;
  if (hipMemsetAsync(m->G, 0, sizeof(float) * grad_floats(m), (hipStream_t)stream) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}

namespace {
// d f1 = (d f2 W2) * [f1 > 0] / (1-p), then d x1 += d f1 W1: two row-skinny launches (f1 is stored post-relu, post-dropout, so
// f1 > 0 <=> kept and pre-activation > 0)
void Pass::skinny_ffn_dx(bool wt) {
  mmda_skinny_args g = sk_dxw(wt, 6 * B, hs, FFN, WS(w.d_f2), hs, WS(w.l2_wT), PP(p.l2_w), WS(w.d_f1), FFN, 0);
  g.gate = WS(w.f1); g.ldgate = FFN; g.gate_scale = p_tf > 0.f ? 1.f / (1.f - p_tf) : 1.f;
  sk_launch(*this, &g, 1);
  g = sk_dxw(wt, 6 * B, FFN, hs, WS(w.d_f1), FFN, WS(w.l1_wT), PP(p.l1_w), WS(w.d_x1), hs, 1);
  sk_launch(*this, &g, 1);
}
// d utt = d z W_proj of the three projections: one row-skinny launch
void Pass::skinny_proj_dx(bool wt) {
  mmda_skinny_args g[3];
  for (int i = 0; i < 3; ++i) {
    const ModP& md = p.mod[i]; const ModW& mw = w.mod[i];
    g[i] = sk_dxw(wt, B, hs, 4 * md.H, WS(w.d_z + i * BH), hs, WS(w.pwT[i]), PP(md.pw), WS(mw.d_utt), 4 * md.H, 0);
  }
  sk_launch(*this, g, 3);
}

// the fusion block's dX chain as the fused row-local stretches (fused_rows.hip): heads' sigmoid' -> d_hfused -> LayerNorm 2, the
// feed-forward pair, and LayerNorm 1 -> ... -> the projection LayerNorms
void Pass::bwd_fusion_fused() {
  {
    FusedBwdC f = {};
    f.B = B; f.hs = hs; f.ncls = c.ncls; f.nb = 1;
    f.tcp = WS(w.tcp); f.scores = WS(w.scores); f.d_tcp = WS(w.d_tcp); f.d_scores = WS(w.d_scores); f.d_logits = WS(w.d_logits);
    // flag join pending: d_tcp is all zeros (no ConfidNet gradients in that mode), but cleared by the side stream's chain, which
    // this launch does not wait for -- NULL reads as zero
    if (m->fj1) f.d_tcp = nullptr;
    // the reconstruction term of stretch A's d_x6 chain, in workgroups of this launch (small batches: both sets fit the chip twice
    // over; MMDA_FUSED_SPLIT=0: inside stretch A as before)
    if (P.rec_hoisted) { f.d_recon = WS(w.d_recon); f.rec_wT = WS(w.rec_wT); f.rec_part = WS(w.rec_part); }
    f.p_cls = p_cls; f.seed = seed; f.site_cls = SITE_CLS; f.reg = m->reg; f.head_w = PP(p.head_w); f.d_hfused = WS(w.d_hfused); f.ln2 = norm2_bwd();
    f.pg_parts = WS(w.pg_parts);
    rc = mmda_fused_bwd_c(&f, s);
  }
  if (P.ffn_fuse_bwd) {
    if (!rc) {
      FusedFfnBwd f = {};
      f.M = 6 * B; f.hs = hs; f.F = FFN; f.S = 32; f.d_f2 = WS(w.d_f2); f.f1 = WS(w.f1);
      f.gate_scale = p_tf > 0.f ? 1.f / (1.f - p_tf) : 1.f; f.l2_wT = WS(w.l2_wT); f.d_f1 = WS(w.d_f1); f.l1_wT = WS(w.l1_wT);
      f.parts = WS(w.ffn_parts);
      rc = mmda_fused_ffn_bwd(&f, s);
    }
  } else {
    skinny_ffn_dx(true);
  }
  if (rc) return;
  FusedBwdA f = {};
  f.B = B; f.hs = hs; f.nhead = NHEAD; f.nb = 1;
  if (P.ffn_fuse_bwd) { f.ffn_parts = WS(w.ffn_parts); f.n_parts = FFN / 32; f.d_x1 = WS(w.d_x1); }
  f.ln1 = norm1_bwd();
  f.d_attn_out = WS(w.d_attn_out); f.out_wT = WS(w.out_wT); f.d_ctx = WS(w.d_ctx);
  f.qkv = WS(w.qkv); f.probs = WS(w.probs); f.d_qkv = WS(w.d_qkv); f.p_tf = p_tf; f.seed = seed; f.site_attn = SITE_ATTN;
  f.in_wT = WS(w.in_wT); f.d_recon = WS(w.d_recon); f.rec_wT = WS(w.rec_wT); f.x6 = WS(w.x6); f.d_x6 = WS(w.d_x6);
  if (P.rec_hoisted) f.rec_part = WS(w.rec_part);
  f.priv_wT = WS(w.priv_wT); f.sh_wT = WS(w.sh_wT); f.d_orig = WS(w.d_orig);
  for (int i = 0; i < 3; ++i) f.lnp[i] = proj_ln_bwd(i);
  f.pg_parts = WS(w.pg_parts);
  if (m->fj1) {
    // Waiting workgroups hold their CU's LDS (104 KB each): with one on every CU the side stream's kernels could not start, and
    // the wait would never end -- on the device only while the stretch leaves most of the chip free (P.fj_device); otherwise the
    // event, here (two launches later than the end of the forward pass, where it used to be: the loss chain is the longer one at
    // large B)
    if (P.fj_device) { f.wait_flag = m->jflags; f.wait_value = m->jval[0]; f.wait_err = m->jflags + 2; }
    else rc = flag_join_fallback(m, s);
    m->fj1 = 0;
  }
  if (!rc) rc = mmda_fused_bwd_a(&f, s);
  if (!P.enc_cut) skinny_proj_dx(true);                  // (d_utt feeds the encoders only)
}

// ... as stand-alone row-skinny launches (MMDA_ROW_FUSE=0, the adversarial discriminator, hidden != 128, or no K-major copies)
void Pass::bwd_fusion_skinny() {
  const bool wt = m->wT_valid != 0;                   // K-major weight copies from this step's forward (side stream, joined there)
  mmda_skinny_args g[8];
  rc = mmda_heads_bwd_task(WS(w.tcp), WS(w.scores), WS(w.d_tcp), WS(w.d_scores), B, c.ncls, WS(w.d_logits), p_cls, seed, SITE_CLS,
                           m->reg != REG_NONE, s);
  g[0] = sk_dxw(wt, B, NC, 6 * hs, WS(w.d_logits), NC, WS(w.head_wT), PP(p.head_w), WS(w.d_hfused), 6 * hs, 0);
  sk_launch(*this, g, 1);
  const mmda_ln_bwd_args l2 = norm2_bwd(), l1 = norm1_bwd();
  if (!rc) rc = mmda_layernorm_bwd(&l2, s);
  skinny_ffn_dx(wt);
  // norm1 + self-attention
  if (!rc) rc = mmda_layernorm_bwd(&l1, s);
  int n = 0;
  g[n++] = sk_dxw(wt, 6 * B, hs, hs, WS(w.d_attn_out), hs, WS(w.out_wT), PP(p.out_w), WS(w.d_ctx), hs, 0);
  if (!c.use_cmd_sim) g[n++] = sk_dxw(wt, 3 * B, 3, hs, WS(w.d_dom), 3, WS(w.d2_wT), PP(p.d2_w), WS(w.d_dom_h), hs, 0);
  sk_launch(*this, g, n);
  if (!rc) rc = mmda_attn_bwd(WS(w.qkv), WS(w.probs), WS(w.d_ctx), S6, B, hs, NHEAD, WS(w.d_qkv), p_tf, seed, SITE_ATTN, s);
  // adversarial branch: the REVERSED gradient into the shared codes (functions.py:17-21)
  if (!c.use_cmd_sim) {
    if (!rc) {
      const mmda_act_params ap = act_params(m, m->training, seed, SITE_RRELU_DISC, true);
      rc = mmda_act_dropout_bwd_p(WS(w.d_dom_h), WS(w.dom_z), WS(w.d_dom_z), 3 * BH, c.act, &ap, p_cls, seed, SITE_DISC, s);
    }
    g[0] = sk_dxw(wt, 3 * B, hs, hs, WS(w.d_dom_z), hs, WS(w.d1_wT), PP(p.d1_w), WS(w.d_x6 + 3 * BH), hs, 1);
    g[0].alpha = -c.reverse_grad_weight;
    sk_launch(*this, g, 1);
  }
  // d_x6[token j] = (d_x6 + d_qkv[j] W_in + d_recon[j % 3] W_rec[j % 3]) * s (1 - s): the q/k/v projection's and the
  // reconstruction's input gradients (the latter flows into BOTH private and shared) and the sigmoid backward, six problems
  for (int j = 0; j < 6; ++j) {
    const int i = j % 3;
    g[j] = sk_dxw(wt, B, 3 * hs, hs, WS(w.d_qkv + (int64_t)j * B * 3 * hs), 3 * hs, WS(w.in_wT), PP(p.in_w), WS(w.d_x6 + j * BH), hs, 1);
    g[j].K2 = hs; g[j].A_2nd = WS(w.d_recon + i * BH); g[j].lda_2nd = hs; g[j].ldb_2nd = hs;
    g[j].B_2nd = wt ? WS(w.rec_wT + (int64_t)i * hs * hs) : PP(p.rec_w + (int64_t)i * hs * hs);
    g[j].dsig = WS(w.x6 + j * BH); g[j].lddsig = hs;
  }
  sk_launch(*this, g, 6);
  // d_orig[i] += d_private[i] W_priv[i] + d_shared[i] W_shared
  for (int i = 0; i < 3; ++i) {
    g[i] = sk_dxw(wt, B, hs, hs, WS(w.d_x6 + i * BH), hs, WS(w.priv_wT + (int64_t)i * hs * hs), PP(p.priv_w + (int64_t)i * hs * hs),
                  WS(w.d_orig + i * BH), hs, 1);
    g[i].K2 = hs; g[i].A_2nd = WS(w.d_x6 + (3 + i) * BH); g[i].lda_2nd = hs; g[i].B_2nd = wt ? WS(w.sh_wT) : PP(p.sh_w); g[i].ldb_2nd = hs;
  }
  sk_launch(*this, g, 3);
  // projections
  if (!rc) {
    mmda_ln_bwd_args l[3];
    for (int i = 0; i < 3; ++i) l[i] = proj_ln_bwd(i);
    rc = mmda_layernorm_bwd_multi(l, 3, s);
  }
  if (!P.enc_cut) skinny_proj_dx(wt);
}

// ... many rows: the tiled generic kernel
void Pass::bwd_fusion_tiled() {
  // heads
  rc = mmda_heads_bwd_task(WS(w.tcp), WS(w.scores), WS(w.d_tcp), WS(w.d_scores), B, c.ncls, WS(w.d_logits), p_cls, seed, SITE_CLS,
                           m->reg != REG_NONE, s);
  lin_dx(*this, fmode, B, NC, 6 * hs, WS(w.d_logits), PP(p.head_w), WS(w.d_hfused), 0);
  // norm2 + FFN
  const mmda_ln_bwd_args l2 = norm2_bwd(), l1 = norm1_bwd();
  if (!rc) rc = mmda_layernorm_bwd(&l2, s);
  {
    // d f1 = (d f2 W2) * [f1 > 0] / (1-p): f1 is stored post-relu, post-dropout, so f1 > 0 <=> kept and pre-activation > 0
    mmda_gemm_args e = {};
    e.gate = WS(w.f1); e.ldgate = FFN; e.gate_scale = p_tf > 0.f ? 1.f / (1.f - p_tf) : 1.f;
    gemm(*this, fmode, 0, 0, 6 * B, FFN, hs, WS(w.d_f2), hs, PP(p.l2_w), FFN, WS(w.d_f1), FFN, nullptr, nullptr, 0, 0, 1, 0, 0, 0, 0, &e);
  }
  lin_dx(*this, fmode, 6 * B, FFN, hs, WS(w.d_f1), PP(p.l1_w), WS(w.d_x1), 1);
  // norm1 + self-attention
  if (!rc) rc = mmda_layernorm_bwd(&l1, s);
  lin_dx(*this, fmode, 6 * B, hs, hs, WS(w.d_attn_out), PP(p.out_w), WS(w.d_ctx), 0);
  if (!rc) rc = mmda_attn_bwd(WS(w.qkv), WS(w.probs), WS(w.d_ctx), S6, B, hs, NHEAD, WS(w.d_qkv), p_tf, seed, SITE_ATTN, s);
  lin_dx(*this, fmode, 6 * B, 3 * hs, hs, WS(w.d_qkv), PP(p.in_w), WS(w.d_x6), 1);
  // adversarial branch: the REVERSED gradient into the shared codes (functions.py:17-21)
  if (!c.use_cmd_sim) {
    lin_dx(*this, fmode, 3 * B, 3, hs, WS(w.d_dom), PP(p.d2_w), WS(w.d_dom_h), 0);
    if (!rc) {
      const mmda_act_params ap = act_params(m, m->training, seed, SITE_RRELU_DISC, true);
      rc = mmda_act_dropout_bwd_p(WS(w.d_dom_h), WS(w.dom_z), WS(w.d_dom_z), 3 * BH, c.act, &ap, p_cls, seed, SITE_DISC, s);
    }
    mmda_gemm_args e = {};
    e.alpha = -c.reverse_grad_weight;
    gemm(*this, fmode, 0, 0, 3 * B, hs, hs, WS(w.d_dom_z), hs, PP(p.d1_w), hs, WS(w.d_x6 + 3 * BH), hs, nullptr, nullptr, 1, 0, 1, 0, 0, 0, 0, &e);
  }
  // reconstruct: d(private+shared) goes to both halves of d_x6
  gemm(*this, fmode, 0, 0, B, hs, hs, WS(w.d_recon), hs, PP(p.rec_w), hs, WS(w.d_x6), hs, nullptr, nullptr, 1, 0, 3, BH, (int64_t)hs * hs, BH);
  gemm(*this, fmode, 0, 0, B, hs, hs, WS(w.d_recon), hs, PP(p.rec_w), hs, WS(w.d_x6 + 3 * BH), hs, nullptr, nullptr, 1, 0, 3, BH,
       (int64_t)hs * hs, BH);
  // sigmoid of private/shared
  if (!rc) rc = mmda_sigmoid_bwd_inplace(WS(w.d_x6), WS(w.x6), 6 * BH, s);
  gemm(*this, fmode, 0, 0, B, hs, hs, WS(w.d_x6), hs, PP(p.priv_w), hs, WS(w.d_orig), hs, nullptr, nullptr, 1, 0, 3, BH, (int64_t)hs * hs, BH);
  lin_dx(*this, fmode, 3 * B, hs, hs, WS(w.d_x6 + 3 * BH), PP(p.sh_w), WS(w.d_orig), 1);
  // projections
  for (int i = 0; i < 3 && !rc; ++i) {
    const ModP& md = p.mod[i]; const ModW& mw = w.mod[i];
    const mmda_ln_bwd_args l = proj_ln_bwd(i);
    rc = mmda_layernorm_bwd(&l, s);
    if (!P.enc_cut) lin_dx(*this, fmode, B, hs, 4 * md.H, WS(w.d_z + i * BH), PP(md.pw), WS(mw.d_utt), 0);
  }
}

// The fusion block's weight gradients, the same list for every form of its dX chain: head, l2, l1, out, in, [d2, d1], rec, priv, sh,
// projections 0-2.  One grouped launch on the side stream (bwd_side_chain) once the dX chain, the critical path, is through.
void Pass::fusion_wgrads() {
  deferring = true;
  lin_dw(*this, fmode, B, NC, 6 * hs, WS(w.d_logits), WS(w.hfused), GG(p.head_w), GG(p.head_b));
  lin_dw(*this, fmode, 6 * B, hs, FFN, WS(w.d_f2), WS(w.f1), GG(p.l2_w), GG(p.l2_b));
  lin_dw(*this, fmode, 6 * B, FFN, hs, WS(w.d_f1), WS(w.x1), GG(p.l1_w), GG(p.l1_b));
  lin_dw(*this, fmode, 6 * B, hs, hs, WS(w.d_attn_out), WS(w.ctx), GG(p.out_w), GG(p.out_b));
  lin_dw(*this, fmode, 6 * B, 3 * hs, hs, WS(w.d_qkv), WS(w.x6), GG(p.in_w), GG(p.in_b));
  if (!c.use_cmd_sim) {
    lin_dw(*this, fmode, 3 * B, 3, hs, WS(w.d_dom), WS(w.dom_h), GG(p.d2_w), GG(p.d2_b));
    lin_dw(*this, fmode, 3 * B, hs, hs, WS(w.d_dom_z), WS(w.x6 + 3 * BH), GG(p.d1_w), GG(p.d1_b));
  }
  mmda_gemm_args e = {};
  e.bias_grad = GG(p.rec_b);      // strideBias = hs: one bias gradient per batched problem
  gemm(*this, fmode, 1, 0, hs, hs, B, WS(w.d_recon), hs, WS(w.rsum), hs, GG(p.rec_w), hs, nullptr, nullptr, 1, 0, 3, BH, BH, (int64_t)hs * hs,
       hs, &e);
  e.bias_grad = GG(p.priv_b);
  gemm(*this, fmode, 1, 0, hs, hs, B, WS(w.d_x6), hs, WS(w.orig), hs, GG(p.priv_w), hs, nullptr, nullptr, 1, 0, 3, BH, BH, (int64_t)hs * hs,
       hs, &e);
  lin_dw(*this, fmode, 3 * B, hs, hs, WS(w.d_x6 + 3 * BH), WS(w.orig), GG(p.sh_w), GG(p.sh_b));
  for (int i = 0; i < 3; ++i)
    lin_dw(*this, fmode, B, hs, 4 * p.mod[i].H, WS(w.d_z + i * BH), WS(w.mod[i].utt), GG(p.mod[i].pw), GG(p.mod[i].pb));
  deferring = false;
}

// side stream: private + shared (the reconstruction's input, needed only by its weight gradient) and every deferred
// weight-gradient GEMM of the fusion block
void Pass::bwd_side_chain(bool pg_pending, const int64_t* t_ids, const int32_t* lengths) {
  void* ss = nullptr;
  rc = side_fork(m, s, &ss);
  if (!rc && m->misc_deferred) {
    // loss values of the step (the forward stretches stored every gradient seed: see mmda_misa::misc_deferred)
    rc = mmda_loss_misc_reg(WS(w.scores), WS(w.tcp), m->misc_deferred, B, c.ncls, nullptr, nullptr, c.ncls == 6, 0, c.conf_weight,
                            WS(w.recon), WS(w.orig), 3 * BH, c.recon_weight, nullptr, nullptr, WS(w.losses), c.diff_weight,
                            c.sim_weight, c.recon_weight, c.conf_weight, c.use_confidNet, m->cls(), m->reg, ss);
    m->misc_deferred = nullptr;
  }
  if (!rc && P.skinny) rc = mmda_add(WS(w.x6), WS(w.x6 + 3 * BH), WS(w.rsum), 3 * BH, ss);
  // the sorted id list of the embedding scatter (see mmda_misa::esort_valid); MMDA_SORT_EARLY=0: made where the scatter runs
  m->esort_valid = 0;
  // (sparse mode without an optimizer step behind this backward: the rows update runs later, in mmda_misa_adam_step, and sorts there)
  if (!rc && P.sort_early && !((P.embed_update == EU_SPARSE || P.embed_deferred) && !opt)) {
    rc = mmda_embed_sort_ids(t_ids, B * w.T, lengths, B, c.vocab, reinterpret_cast<unsigned*>(WS(w.esort)), ss);
    if (!rc && ss != s) {
      hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)ss, m->jflags + 3, ++m->esort_val);
      if (hipGetLastError() != hipSuccess) rc = MMDA_ELAUNCH;
    }
    m->esort_valid = rc ? 0 : (ss != s ? 2 : 1);
  }
  if (!rc && pg_pending) {
    // gamma / beta gradients of the five LayerNorms the fused stretches walked: per-sample partials added in sample order
    float* dg[FUSED_PG_SLOTS] = {GG(p.n2_w), GG(p.n1_w), GG(p.mod[0].plw), GG(p.mod[1].plw), GG(p.mod[2].plw)};
    float* db[FUSED_PG_SLOTS] = {GG(p.n2_b), GG(p.n1_b), GG(p.mod[0].plb), GG(p.mod[1].plb), GG(p.mod[2].plb)};
    rc = mmda_fused_pg_finish(WS(w.pg_parts), B, hs, dg, db, ss);
  }
  if (!rc && !deferred.empty()) rc = mmda_gemm_grouped(deferred.data(), (int)deferred.size(), ss);
  deferred.clear();
  // the bf16 operand copies that only the weight-gradient GEMMs read (hseq of both layers, nt form: transposed layer-2 inputs): here,
  // where the side stream is idle beside the layer-2 recurrence, instead of in front of the loss kernels of the forward pass
  if (!rc && P.bfg && w.T > 0 && !P.enc_cut) {           // (a cut step runs no encoder weight-gradient GEMM)
    mmda_convert_job cj[16];
    const int nj = backward_only_jobs(m, cj);
    rc = mmda_convert_bf16(cj, nj, ss);
  }
  // (Clip + Adam of the embedding rows this batch does not touch does not belong here: as a burst of the full grid beside the layer-2
  // recurrence its 170 MB stream slows the recurrence's hand-offs and the step by 14 us at B=32; behind the early optimizer pass, by
  // 68 us.  It runs as a trickle of a few workgroups under the forward pass instead: mmda_misa::bg)
}

// encoder layer l, top layer first: the backward recurrence, then the weight and input gradient GEMMs of the three modalities.
// Layer 2's weight-gradient GEMMs run beside the layer-1 recurrent kernel on the side stream (faster than holding them back for
// one grouped launch with layer 1's after it).  The wave-autonomous recurrence runs one wave on each of ~110 CUs,
// raises its priority and reserves those CUs' whole LDS, so the GEMM's workgroups land on the other ~145 CUs; what the two still
// share is L2 and fabric bandwidth (the recurrence slows by ~30 us, the GEMMs' ~65 us leave the critical path).
void Pass::bwd_encoder_layer(int l, const float* const* xin, const int64_t* t_ids, const int32_t* lengths) {
  mmda_lstm_desc desc[3];
  for (int i = 0; i < 3; ++i) desc[i] = lstm_desc(m, i, l, true, P.gm, P.want_c);
  // The wave-autonomous gate-minor kernel emits the gate gradients as bf16 (the operand of the input-gradient GEMM) -- and only
  // as bf16: every consumer of dG in this mode is a bf16 GEMM (the transposed operand is re-laid-out from it).  The other
  // kernels (barrier form: H > 320, ablation switches) write fp32 `gates` as before.
  if (P.kdg)
    for (int i = 0; i < 3; ++i) { desc[i].dg_bf16 = WS(w.mod[i].rnn[l].dgb); desc[i].dg_bf16_only = 1; }
  m->epoch += (unsigned)T + 2u;
  // the forward pass skipped the streaming backward packing because the resident-weights kernels were going to run: they must
  if (!P.want_b && !mmda_lstm_resident_applicable(mode, 3, desc, B, T, 1)) { rc = MMDA_EINVAL; return; }
  ev_rec(m, m->ev_bwd, l == 1 ? 2 : 3, 0, s);
  rc = mmda_lstm_bwd(mode, 3, desc, B, T, lengths, s);
  ev_rec(m, m->ev_bwd, l == 1 ? 2 : 3, 1, s);
  if (rc) return;
  // All weight / input gradient GEMMs of this layer (three modalities) are independent.  Layer 2: d(normed) feeds the
  // next recurrent kernel (main stream); its weight gradients run on the side stream underneath that kernel.
  const bool bfg = P.bfg, bf_hh = bfg && (B % 8) == 0;        // the time-shifted views of dG^T / hseq^T start B elements into a row
  std::vector<mmda_gemm_bf16_args> bmain, bside;
  // gate gradients -> bf16: transposed (A of every dW) and, where an input gradient is needed and the recurrent kernel did not
  // write it itself, plain (A of dX).  Layer 2 with the kernel-written plain copy: only the weight-gradient GEMMs (side stream)
  // read the transposed one, so the conversion goes to the side stream with them.
  const bool frozen = P.embed_update == EU_FROZEN;            // no gradient w.r.t. the embedding rows: text layer 1 has no dX product
  mmda_convert_job dgj[3];
  for (int i = 0; i < 3; ++i) {
    const RnnP& r = p.mod[i].rnn[l]; const ModW& mw = w.mod[i]; const RnnW& rw = mw.rnn[l];
    const bool plain = (l == 1 || (i == 0 && !frozen)) && !P.kdg;
    dgj[i] = mmda_convert_job{WS(mw.gates[l]), 8 * r.H, R, 8 * r.H, nullptr, plain ? WS(rw.dgb) : nullptr, plain ? r.ldG : 0, WS(rw.dgbT),
                              w.ldR};
    if (P.kdg) { dgj[i].src = WS(rw.dgb); dgj[i].ld = r.ldG; dgj[i].src_bf16 = 1; }
  }
  const bool tn = P.tn_wgrad;            // weight gradients straight from dG / inputs / hseq as they lie (no dG^T); implies kdg
  const bool dg_on_side = P.kdg && l == 1 && m->use_side && !tn;
  if (bfg && !dg_on_side && !tn) {
    rc = mmda_convert_bf16(dgj, 3, s);
    if (rc) return;
  }
  deferring = (l == 1);
  group_begin(*this);
  for (int i = 0; i < 3; ++i) {
    const RnnP& r = p.mod[i].rnn[l]; const ModW& mw = w.mod[i]; const RnnW& rw = mw.rnn[l];
    const int H = r.H, G8 = 8 * H;
    const float* dG = WS(mw.gates[l]);
    const float* in = l == 0 ? xin[i] : WS(mw.normed);
    std::vector<mmda_gemm_bf16_args>& wq = (l == 1) ? bside : bmain;      // weight gradients: side stream for layer 2
    const unsigned short* dgT = reinterpret_cast<const unsigned short*>(WS(rw.dgbT));
    const unsigned short* hT = reinterpret_cast<const unsigned short*>(WS(rw.hbT));
    // dW_ih (both directions stacked); db_ih = db_hh = column sums of dG ride along as a virtual ones-column
    if (bfg) {
      mmda_gemm_bf16_args g = {};
      g.M = G8; g.N = r.D; g.K = R; g.A = dgT; g.lda = w.ldR; g.B = WS(rw.xbT); g.ldb = w.ldR; g.C = gW_ih(m, i, l); g.ldc = r.D;
      g.accumulate = 1; g.bias_grad = gB_ih(m, i, l); g.bias_grad2 = gB_hh(m, i, l); g.perm_m_H = P.gm ? H : 0;
      if (tn) { g.tn = 1; g.A = WS(rw.dgb); g.lda = r.ldG; g.B = WS(rw.xb); g.ldb = r.ldD; }
      wq.push_back(g);
    } else {
      mmda_gemm_args e = {};
      e.bias_grad = gB_ih(m, i, l); e.bias_grad2 = gB_hh(m, i, l);
      gemm(*this, mode, 1, 0, G8, r.D, R, dG, G8, in, r.D, gW_ih(m, i, l), r.D, nullptr, nullptr, 1, 0, 1, 0, 0, 0, 0, &e);
    }
    // dW_hh: forward direction pairs dG[t] with h[t-1]; reverse direction pairs dG[t] with h[t+1] (zero past len)
    if (T > 1) {
      if (bf_hh) {
        mmda_gemm_bf16_args g = {};
        g.M = 4 * H; g.N = H; g.K = (T - 1) * B; g.lda = w.ldR; g.ldb = w.ldR; g.ldc = H; g.accumulate = 1;
        g.perm_m_H = P.gm ? H : 0;
        if (tn) {
          // rows of dG / hseq are (t, b): the forward direction pairs rows t B + b of dG with rows (t - 1) B + b of h, the reverse
          // direction rows t B + b with rows (t + 1) B + b
          const unsigned short* dg = reinterpret_cast<const unsigned short*>(WS(rw.dgb));
          const unsigned short* h0 = reinterpret_cast<const unsigned short*>(WS(rw.hbp[0]));
          const unsigned short* h1 = reinterpret_cast<const unsigned short*>(WS(rw.hbp[1]));
          g.tn = 1; g.lda = r.ldG; g.ldb = r.ldH;
          g.A = dg + (int64_t)B * r.ldG; g.B = h0; g.C = gW_hh(m, i, l, 0);
          wq.push_back(g);
          g.A = dg + 4 * H; g.B = h1 + (int64_t)B * r.ldH; g.C = gW_hh(m, i, l, 1);
          wq.push_back(g);
        } else {
          g.A = dgT + B; g.B = hT; g.C = gW_hh(m, i, l, 0);
          wq.push_back(g);
          g.A = dgT + (int64_t)4 * H * w.ldR; g.B = hT + (int64_t)H * w.ldR + B; g.C = gW_hh(m, i, l, 1);
          wq.push_back(g);
        }
      } else {
        const float* hs_ = WS(mw.hseq[l]);
        gemm(*this, mode, 1, 0, 4 * H, H, (T - 1) * B, dG + (int64_t)B * G8, G8, hs_, 2 * H, gW_hh(m, i, l, 0), H, nullptr, nullptr, 1);
        gemm(*this, mode, 1, 0, 4 * H, H, (T - 1) * B, dG + 4 * H, G8, hs_ + (int64_t)B * 2 * H + H, 2 * H, gW_hh(m, i, l, 1), H, nullptr,
             nullptr, 1);
      }
    }
    // d(normed) = dG W_ih (layer 2) / d(embedding rows) (text layer 1)
    if (l == 1 || i == 0) {
      float* dst = l == 1 ? WS(mw.d_normed) : WS(mw.d_x);
      const bool skip = l == 0 && frozen;                    // frozen table: the text layer-1 dX product is not run
      if (bfg) {
        mmda_gemm_bf16_args g = {};
        g.M = R; g.N = r.D; g.K = G8; g.A = WS(rw.dgb); g.lda = r.ldG; g.B = WS(rw.wbT); g.ldb = r.ldG; g.C = dst; g.ldc = r.D;
        if (!skip) bmain.push_back(g);
      } else {
        // (left out of a frozen step's group, but counted when its split-K is sized: the weight gradients beside it keep their slices)
        absent_next = skip;
        gemm(*this, mode, 0, 0, R, r.D, G8, dG, G8, rW_ih(m, i, l), r.D, dst, r.D);
      }
    }
  }
  group_end(*this);
  deferring = false;
  if (!rc && !bmain.empty()) rc = mmda_gemm_bf16_grouped(bmain.data(), (int)bmain.size(), s);
  if (rc) return;
  if (l == 1) {
    // the inter-layer LayerNorm backward gives d(hseq of layer 1): input gradients on the main stream (they feed the next
    // recurrent kernel); gamma/beta gradients and this layer's weight-gradient GEMMs on the side stream underneath it
    mmda_ln_bwd_args lb[3];
    for (int i = 0; i < 3; ++i) {
      const ModP& md = p.mod[i]; const ModW& mw = w.mod[i];
      lb[i] = mmda_ln_bwd_args{};
      lb[i].rows = R; lb[i].n = 2 * md.H; lb[i].dy = WS(mw.d_normed); lb[i].x = WS(mw.hseq[0]); lb[i].gamma = PP(md.ln_w);
      lb[i].mean = WS(mw.ln_mean); lb[i].rstd = WS(mw.ln_rstd); lb[i].d_x = WS(mw.d_hseq1);
    }
    // (the input-gradient launch goes out BEFORE the fork: it reads the LayerNorm weights, which the early optimizer step below may
    // update on the side stream -- the fork orders the side stream behind it)
    // 16-byte form (norm.hip): the d_x launch leaves the gamma / beta gradients as per-block partials on its way (it reads dy and x
    // anyway) and the side stream only adds them up -- instead of a second pass over dy and x there (100 us at B = 256)
    const bool ln_split = mmda_ln_bwd_parts_applies(lb, 3) &&
                          mmda_ln_parts_floats(lb, 3) <= (int64_t)512 * 2 * 2 * (p.mod[0].H + p.mod[1].H + p.mod[2].H);
    if (ln_split) {
      for (int i = 0; i < 3; ++i) { lb[i].dgamma = GG(p.mod[i].ln_w); lb[i].dbeta = GG(p.mod[i].ln_b); }
      rc = mmda_ln_bwd_parts(lb, 3, WS(w.ln_parts), s);
    } else {
      rc = mmda_layernorm_bwd_multi(lb, 3, s);
    }
    void* ss = nullptr;
    if (!rc) rc = side_fork(m, s, &ss);
    for (int i = 0; i < 3; ++i) { lb[i].dgamma = GG(p.mod[i].ln_w); lb[i].dbeta = GG(p.mod[i].ln_b); if (!ln_split) lb[i].d_x = nullptr; }
    if (!rc && dg_on_side) rc = mmda_convert_bf16(dgj, 3, ss);
    if (!rc) rc = ln_split ? mmda_ln_parts_finish(lb, 3, WS(w.ln_parts), ss) : mmda_layernorm_param_grads(lb, 3, ss);
    if (!rc && !deferred.empty()) rc = mmda_gemm_grouped(deferred.data(), (int)deferred.size(), ss);
    const bool l2_early = !bside.empty();
    if (!rc && l2_early) { rc = mmda_gemm_bf16_grouped(bside.data(), (int)bside.size(), ss); bside.clear(); }
    deferred.clear();
    // Everything issued so far on either stream is final for the fusion block, the LayerNorms and -- when its weight-gradient
    // GEMMs just went out and no GRU re-layout follows -- layer 2: data-parallel ranks may start reducing that prefix now,
    // beside the layer-1 recurrence (mmda_misa_wait_early_grads).
    if (rc) return;
    if (!m->ev_early && hipEventCreateWithFlags(&m->ev_early, hipEventDisableTiming) != hipSuccess) rc = MMDA_ELAUNCH;
    if (!rc && hipEventRecord(m->ev_early, (hipStream_t)ss) != hipSuccess) rc = MMDA_ELAUNCH;
    m->early_floats = (l2_early && !is_gru(m) && P.bfg) ? p.rnn1_begin : p.rnn2_begin;
    m->early_valid = 1;
    // Single-GPU fused step: clip + Adam of that prefix right here, beside the layer-1 recurrence (nothing issued after this
    // point reads those fp32 parameters: the remaining GEMMs of a bf16 step read bf16 copies made in the forward pass, and in
    // the other modes the prefix ends in front of the recurrent layers).  The side stream is a real second stream only when
    // use_side is on; otherwise this is simply the same work in front of the recurrence.
    if (!rc && opt && m->early_floats > 0 && m->M1 && m->V1) {
      // (frozen parameters: over the prefix's trainable runs -- the prefix counts as stepped even where none of it trains)
      rc = bucket_adam(m, 0, m->early_floats, nullptr, opt->lr, opt->clip, opt->grad_scale, opt->step, kNoWait, ss);
      if (!rc) m->adam_early_done = m->early_floats;
    }
  } else {
    bwd_text_rows(t_ids, lengths);
  }
}

// The sorted id list that bwd_side_chain made for this pass, or nullptr (taken once).  Made on the side stream: its word, waited for
// by one wave in front of the launch that reads the list.
const unsigned* Pass::take_sorted() {
  if (!m->esort_valid) return nullptr;
  if (m->esort_valid == 2) {
    hipLaunchKernelGGL(flag_wait_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, m->jflags + 3, m->esort_val, m->jflags + 2);
    if (hipGetLastError() != hipSuccess) rc = MMDA_ELAUNCH;
  }
  m->esort_valid = 0;
  return reinterpret_cast<const unsigned*>(WS(w.esort));
}

// The text rows' end of the pass, behind layer 1: d_x_t goes where embed_update sends it.  Sparse and deferred tables take their rows update
// here, behind an optimizer step only (`opt`); otherwise the pass stops at d_x_t, the rows stay pending for mmda_misa_adam_step.
void Pass::bwd_text_rows(const int64_t* t_ids, const int32_t* lengths) {
  const float* dx = WS(w.mod[0].d_x);
  if (P.embed_update == EU_SPARSE || P.embed_deferred) {
    m->eu.take();
    if (!opt) { m->eu.set(t_ids, lengths); return; }
  }
  if (P.embed_update == EU_FROZEN) return;
  // the list, with the sorted form of it if this pass made one; embed_rows.hip picks the form the sums take
  const EmbedList list{t_ids, take_sorted(), R, c.d_t, dx, lengths, B};
  if (rc) return;
  if (P.embed_update == EU_SPARSE) {
    // SparseAdam on the rows the batch touches (common.h)
    SparseAdamArgs ad;
    rc = mmda_sparse_adam_args(&ad, PP(p.embed), m->M1 ? m->M1 + p.embed : nullptr, m->V1 ? m->V1 + p.embed : nullptr, c.vocab, opt->lr,
                               m->adam.beta1, m->adam.beta2, m->adam.eps, opt->clip, opt->grad_scale, opt->step);
    if (!rc) rc = mmda_embed_list_sparse_adam(ad, list, s);
  } else if (P.embed_deferred) {
    // dense Adam's step for the rows the batch touches (common.h: RowDenseAdam); every other row takes it when it is next needed
    if (!m->M1 || !m->V1) { rc = MMDA_EINVAL; return; }
    rc = deferred_apply(m, t_ids, list.sorted, lengths, opt->lr, m->adam.beta1, m->adam.beta2, m->adam.eps, opt->clip, opt->grad_scale,
                        opt->step, false, s);
  } else {
    // the gradient w.r.t. the embedding rows, scattered densely into embed.weight.grad (sparse=False)
    rc = mmda_embed_list_add(GG(p.embed), list, c.vocab, s);
  }
}
}  // namespace

namespace {
// The backward pass.  The batch (ids / v / a / lengths) is read only by what an encoder cut skips -- the encoder layers, the sorted id
// list, the scatter -- so a step from the encoder cache, which has no batch, passes NULLs: it must be a cut pass planned by a cached
// forward.
// opt: the optimizer step behind this pass, which it may start (nullptr: none, the pass stops at the gradients).
int backward_pass(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths, const OptStep* opt,
                  void* stream) {
  if (check_ready(m) || !m->G) return MMDA_EINVAL;
  if (m->plan.inf) return MMDA_EINVAL;                  // the last forward was an evaluation pass: nothing was stashed
  if ((!t_ids || !v || !a || !lengths) && !(m->plan.enc_cached && m->plan.enc_cut)) return MMDA_EINVAL;
  if (m->plan.enc_cached && !m->plan.enc_cut) return MMDA_EINVAL;      // (a cached forward that trains is a cut one: cannot happen)
  // the trainable set changed behind that forward: a cut pass computes no encoder gradient (and may have stashed nothing)
  if (m->plan.enc_cut && !encoder_cut(m)) return MMDA_EINVAL;
  if (masked(m) && opt) { const int rr = runs_ready(m, stream); if (rr) return rr; }
  m->early_valid = 0; m->adam_early_done = 0;
  Pass x(m, stream, nullptr, opt);
  const StepPlan& P = m->plan;
  // the fused stretches read the K-major weight copies this step's forward made (side stream, joined there)
  const bool row_fuse = P.row_fuse && m->wT_valid;
  if (m->fj1 && !row_fuse) { x.rc = flag_join_fallback(m, stream); m->fj1 = 0; if (x.rc) return x.rc; }     // (no kernel here waits on the device)
  if (row_fuse) x.bwd_fusion_fused();
  else if (P.skinny) x.bwd_fusion_skinny();
  else x.bwd_fusion_tiled();
  x.fusion_wgrads();
  if (x.rc) return x.rc;
  x.bwd_side_chain(row_fuse, t_ids, lengths);
  const float* xin[3] = {WS(m->lay.mod[0].x), v, a};
  // Encoder cut: the pass ends here.  No early optimizer pass, no ev_early, no sorted id list and no flag word of this pass exist,
  // so the join below is the event's (adam_early_done stays 0) and no kernel waits for a word that nobody sets; the recurrent
  // layers' ranges of the gradient bucket hold what the clear left.
  for (int l = 1; l >= 0 && !x.rc && !P.enc_cut; --l) x.bwd_encoder_layer(l, xin, t_ids, lengths);
  if (x.rc) return x.rc;
  if (!m->ev.empty() && !P.enc_cached) { if (m->ev_seen_b % m->ev_stride == 0) m->ev_bwd++; m->ev_seen_b++; }
  // every gradient is complete on `stream` when backward returns -- or, in a fused training step whose last optimizer launch can
  // wait on the device (see mmda_misa::jflags), when that launch completes
  // (only where every gradient the side stream computes lies in the prefix it also stepped -- the bf16 step, whose layer-2 weight
  //  gradients ran there in front of the early optimizer pass: the launch that waits READS the rest of the bucket before it waits)
  if (P.fj_on && opt && !is_gru(m) && m->side_pending && m->jflags && m->adam_early_done > 0 &&
      m->adam_early_done == m->par.rnn1_begin) {
    // (the background pass over the table joins here too: the word is set behind it, and the main stream pays nothing)
    x.rc = bg_join(m, m->side);
    if (!x.rc) x.rc = side_flag_signal(m, 1);
    m->fj2 = x.rc ? 0 : 1;
    return x.rc;
  }
  x.rc = side_join(m, stream);
  if (!x.rc && is_gru(m) && !P.enc_cut) {      // fold the four-slot weight gradients into the torch-layout gradient buffer
    mmda_gru_pad_job gj[MMDA_GRU_PAD_MAX];
    int n = gru_jobs(m, m->G, true, gj);
    x.rc = mmda_gru_unpad_grads(gj, n, stream);
  }
  return x.rc;
}
}  // namespace

extern "C" int mmda_misa_backward(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                                  void* stream) {
  if (!t_ids || !v || !a || !lengths) return MMDA_EINVAL;
  return backward_pass(m, t_ids, v, a, lengths, nullptr, stream);
}

extern "C" int mmda_misa_timing_end(mmda_misa* m) {
  if (!m) return MMDA_EINVAL;
  for (hipEvent_t e : m->ev) (void)hipEventDestroy(e);
  m->ev.clear(); m->ev_steps = m->ev_fwd = m->ev_bwd = 0; m->ev_seen_f = m->ev_seen_b = 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_timing_stride(mmda_misa* m, int stride) {
  if (!m || stride < 1) return MMDA_EINVAL;
  m->ev_stride = stride;
  return MMDA_OK;
}
extern "C" int mmda_misa_timing_begin(mmda_misa* m, int max_steps) {
  if (!m || max_steps <= 0 || max_steps > 4096) return MMDA_EINVAL;
  mmda_misa_timing_end(m);
  m->ev.resize((size_t)max_steps * 8);
  // (timing events only: without the system-scope fence -- cache write-back and invalidation -- a default event performs when it is
  //  recorded, which is what hipEventDisableSystemFence is for: a sampled step costs the run half as much)
  for (auto& e : m->ev)
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return MMDA_ELAUNCH;
  m->ev_steps = max_steps;
  m->ev_done.assign((size_t)max_steps * 4, 0);
  return MMDA_OK;
}
extern "C" int mmda_misa_timing_rotate(mmda_misa* m, int on) {
  if (!m) return MMDA_EINVAL;
  m->ev_rotate = on ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_timing_collect(mmda_misa* m, float mean_ms[4], int* steps) {
  if (!m || !mean_ms || m->ev.empty()) return MMDA_EINVAL;
  int n = m->ev_fwd < m->ev_bwd ? m->ev_fwd : m->ev_bwd;
  if (n > m->ev_steps) n = m->ev_steps;
  double acc[4] = {0, 0, 0, 0};
  int cnt[4] = {0, 0, 0, 0};
  for (int s = 0; s < n; ++s)
    for (int k = 0; k < 4; ++k) {
      if ((size_t)(s * 4 + k) >= m->ev_done.size() || !m->ev_done[s * 4 + k]) continue;      // (rotation: one launch per sampled step)
      float ms = 0.f;
      if (hipEventSynchronize(m->ev[(s * 4 + k) * 2 + 1]) != hipSuccess) return MMDA_ELAUNCH;
      if (hipEventElapsedTime(&ms, m->ev[(s * 4 + k) * 2], m->ev[(s * 4 + k) * 2 + 1]) != hipSuccess) return MMDA_ELAUNCH;
      acc[k] += ms; cnt[k]++;
    }
  int least = n;
  for (int k = 0; k < 4; ++k) { mean_ms[k] = cnt[k] > 0 ? (float)(acc[k] / cnt[k]) : 0.f; least = cnt[k] < least ? cnt[k] : least; }
  if (steps) *steps = least;                            // samples behind every mean (the least-sampled launch)
  return MMDA_OK;
}

// =============================================================================================== optimizer / step
namespace {
// sparse table: the rows of the backward that just ran (d_x_t is workspace: the next micro-batch overwrites it) go to the caller's list
int accum_append_rows(mmda_misa* m, const RowList& l, void* stream) {
  if (!m->eu.on || !m->ws || m->lay.T <= 0 || !l.ids || !l.rows) return MMDA_EINVAL;
  const PendingRows r = m->eu.take();                   // (a later mmda_misa_adam_step must not apply these rows again)
  return mmda_embed_rows_append(l.ids, l.rows, l.used, l.capacity, r.ids, WS(m->lay.mod[0].d_x), m->lay.B * m->lay.T, m->cfg.d_t, r.lengths, m->lay.B, stream);
}
bool accum_ready(const mmda_misa* m) { return m && m->P && m->G && !m->df_row_step; }
// sparse table: a backward is pending and the list holds its T B rows behind the `used` it already has (dense / frozen: no list)
bool accum_list_ok(const mmda_misa* m, const RowList& l) {
  if (m->embed_update != EU_SPARSE) return true;
  const int64_t R = (int64_t)m->lay.B * m->lay.T;
  return m->eu.on && m->ws && m->lay.T > 0 && l.ids && l.rows && l.used >= 0 && l.used <= l.capacity && R <= l.capacity - l.used &&
         l.used + R <= INT32_MAX;
}

// What every optimizer step is checked for in front of its first launch, so that a refused call changes nothing
int opt_step_refused(const mmda_misa* m, const OptStep& o) {
  if (!m->P || !m->G || !m->M1 || !m->V1 || o.step < 1 || (o.norm && !m->ws)) return MMDA_EINVAL;
  return adam_settings_refused(m) ? MMDA_EINVAL : MMDA_OK;
}

// The optimizer part of a step, from bucket offset lo (an early pass stepped what lies in front of it): the run table where parameters
// are frozen, the norm, clamp + Adam over [lo, grad_floats) -- w: that launch waits for the side stream's word -- and the table's rows
// that are still to be updated: the accumulated step's list (sparse table), or the rows a backward left pending (sparse, deferred).
// (Behind a fused step nothing is pending: bwd_text_rows takes m->eu whenever it is handed a step, and a cut pass, which does not get
// that far, needs a frozen or plain dense table (encoder_cut), where the rows part does not apply.)
int opt_step(mmda_misa* m, const OptStep& o, int64_t lo, const FlagWait& w, const RowList* list, void* stream) {
  int rc = masked(m) ? runs_ready(m, stream) : MMDA_OK;
  if (!rc && o.norm) rc = bucket_norm(m, o.acc, o.grad_scale, stream);
  if (!rc) rc = bucket_adam(m, lo, grad_floats(m), o.acc, o.lr, o.clip, o.grad_scale, o.step, w, stream, o.norm ? m->ws + m->lay.gnorm + 1 : nullptr);
  if (rc) return rc;
  float* const p = PP(m->par.embed); float* const m1 = m->M1 + m->par.embed; float* const v1 = m->V1 + m->par.embed; const mmda_adam_opts& h = m->adam;
  if (m->embed_update == EU_SPARSE && list) {
    const int n = (int)(list->used + (int64_t)m->lay.B * m->lay.T);
    rc = accum_append_rows(m, *list, stream);
    // SparseAdam on the rows any micro-batch touched, sums in list order (micro-batch major); padding went in as id -1
    if (!rc) rc = mmda_embed_rows_sparse_adam(p, m1, v1, list->ids, n, m->cfg.d_t, list->rows, nullptr, 0, m->cfg.vocab, o.lr, h.beta1, h.beta2,
                                              h.eps, o.clip, o.grad_scale, o.step, stream);
  } else if (m->embed_update == EU_SPARSE && m->eu.on) {
    // the touched rows of the last backward: coalesce, scale, clamp, SparseAdam (the clamp applies to the coalesced sum)
    const PendingRows r = m->eu.take();
    if (!m->ws || m->lay.T <= 0) return MMDA_EINVAL;
    rc = mmda_embed_rows_sparse_adam(p, m1, v1, r.ids, m->lay.B * m->lay.T, m->cfg.d_t, WS(m->lay.mod[0].d_x), r.lengths, m->lay.B, m->cfg.vocab, o.lr, h.beta1,
                                     h.beta2, h.eps, o.clip, o.grad_scale, o.step, stream);
  } else if (m->embed_update == EU_DENSE && m->df_row_step && m->eu.on) {
    rc = mmda_misa_embed_deferred_step(m, o.lr, h.beta1, h.beta2, h.eps, o.clip, o.grad_scale, o.step, stream);
  }
  return rc;
}
}  // namespace

extern "C" int mmda_misa_adam_step(mmda_misa* m, float lr, float clip, float grad_scale, int step, void* stream) {
  if (!m) return MMDA_EINVAL;
  const OptStep o{lr, clip, grad_scale, step, nullptr, m->clip_norm > 0.f};
  const int rc = opt_step_refused(m, o);
  return rc ? rc : opt_step(m, o, 0, kNoWait, nullptr, stream);
}

// ---- accumulated steps (accum_steps > 1): the micro-batch is mmda_misa_train_step(do_adam = 0); what happens to its gradients is here
extern "C" int mmda_misa_grad_accumulate(mmda_misa* m, float* acc, int first, int64_t* list_ids, float* list_rows, int64_t list_used,
                                         int64_t list_capacity, void* stream) {
  const RowList l{list_ids, list_rows, list_used, list_capacity};
  if (!accum_ready(m) || !acc || !accum_list_ok(m, l)) return MMDA_EINVAL;
  int rc = mmda_grad_accumulate(acc, m->G, grad_floats(m), first, stream);
  if (!rc && m->embed_update == EU_SPARSE) rc = accum_append_rows(m, l, stream);
  return rc;
}

extern "C" int mmda_misa_adam_step_accumulated(mmda_misa* m, const float* acc, int64_t* list_ids, float* list_rows, int64_t list_used,
                                               int64_t list_capacity, float lr, float clip, float grad_scale, int step, void* stream) {
  const RowList l{list_ids, list_rows, list_used, list_capacity};
  if (!accum_ready(m) || !accum_list_ok(m, l)) return MMDA_EINVAL;
  const OptStep o{lr, clip, grad_scale, step, acc, m->clip_norm > 0.f};
  const int rc = opt_step_refused(m, o);
  return rc ? rc : opt_step(m, o, 0, kNoWait, &l, stream);
}

namespace {
// One training step: from a batch (t_ids, v, a, lengths; labels `emo`), or -- eb != nullptr -- from the encoder cache, whose forward
// gathers the labels into `emo` itself.  The two differ in their forward pass and in the batch the backward pass is handed, nowhere else.
// (the body of train_step below, which closes it: whatever this returns, the background pass over the table is joined)
int train_step_body(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths, const mmda_encoded_batch* eb,
                    float* emo_gathered, const float* emo, int training, uint64_t seed, int do_adam, float lr, float clip, int step,
                    void* stream) {
  // the gradient bucket is cleared on the side stream beside the forward pass's fusion block (not at the start of the step: the
  // side stream's first job there, packing W_hh, is what the first recurrent kernel waits for)
  if (check_ready(m) || !m->G) return MMDA_EINVAL;
  // clip_norm: no update may precede the norm, so the backward pass runs as it does without an optimizer step (no early pass, event
  // join); the norm and one launch over the whole bucket follow it
  const OptStep o{lr, clip, 1.0f, step, nullptr, do_adam && m->clip_norm > 0.f};
  const bool early = do_adam && !o.norm;
  int rc = do_adam ? opt_step_refused(m, o) : MMDA_OK;
  if (!rc && do_adam && masked(m)) rc = runs_ready(m, stream);     // frozen parameters: the run table is there before the first launch
  if (rc) return rc;
  m->inference = 0;                                     // a training step always stashes (but for the encoders of a cut step)
  m->zero_grad_pending = m->lay.T > 0 ? 1 : 0;
  m->eager_done = 0; m->misc_deferred = nullptr;
  m->fj1 = m->fj2 = 0;
  // opt: the kind of step that may run the background pass over the table (plan_step decides): from a batch, the native Adam behind it, no norm
  const StepRequest req{true, emo, (early && !eb) ? &o : nullptr, eb != nullptr};
  rc = m->zero_grad_pending ? MMDA_OK : mmda_misa_zero_grad(m, stream);
  if (!rc) rc = eb ? forward_encoded(m, req, eb, emo_gathered, training, seed, stream) : forward_pass(m, req, t_ids, v, a, lengths, training, seed, stream);
  if (rc) return rc;
  if (m->zero_grad_pending) return MMDA_ELAUNCH;        // forward() always reaches its fusion block
  rc = mmda_misa_losses(m, emo, 1, stream);
  if (rc) return rc;
  // (the early optimizer pass beside the layer-1 recurrence: faster than one launch for the whole bucket at the end)
  rc = backward_pass(m, t_ids, v, a, lengths, early ? &o : nullptr, stream);
  if (rc) return rc;
  if (m->fj1) { rc = flag_join_fallback(m, stream); m->fj1 = 0; if (rc) return rc; }      // (no stretch took it over: cannot happen)
  if (m->fj2 && !early) { rc = flag_join_fallback(m, stream); m->fj2 = 0; if (rc) return rc; }
  if (!do_adam) return MMDA_OK;
  // the rest of the bucket (layer-1 recurrent layers, embedding -- or everything, if the backward pass stepped nothing early; a sparse
  // or frozen table: the launch ends in front of it); flag join: it does not complete before the side stream's chain has
  const bool fj = m->fj2 != 0;
  m->fj2 = 0;
  const FlagWait w = fj ? FlagWait{m->jflags + 1, m->jval[1], m->jflags + 2} : kNoWait;
  if (!m->bg_active) return opt_step(m, o, m->adam_early_done, w, nullptr, stream);
  // The background pass stepped the table rows this batch does not index: the launch covers the rest of the bucket in front of the
  // table and the rows whose stamp is this step's, which read the scattered gradient -- one launch, as ever.  (Such a step has no run
  // table, no norm, no accumulator and no pending rows: plan_step.)
  const int64_t lo = m->adam_early_done;
  return mmda_adam_tail_launch(m->P + lo, m->G + lo, m->M1 + lo, m->V1 + lo, m->par.embed - lo, bg_table(m), bg_hyper(m, o), w, stream);
}

int train_step(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths, const mmda_encoded_batch* eb,
               float* emo_gathered, const float* emo, int training, uint64_t seed, int do_adam, float lr, float clip, int step,
               void* stream) {
  if (m) m->bg_active = 0;
  const int rc = train_step_body(m, t_ids, v, a, lengths, eb, emo_gathered, emo, training, seed, do_adam, lr, clip, step, stream);
  // Where the side stream did not take the pass's join into its flag word (fp32 step, MMDA_FLAG_JOIN=0, GRU, no early optimizer pass,
  // a step that failed half-way), the caller's stream waits for it here, behind the closing launch.
  const int rj = (m && m->bg_pending) ? bg_join(m, stream) : MMDA_OK;
  return rc ? rc : rj;
}
}  // namespace

extern "C" int mmda_misa_train_step(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                                    const float* emo, int training, uint64_t seed, int do_adam, float lr, float clip, int step,
                                    void* stream) {
  return train_step(m, t_ids, v, a, lengths, nullptr, nullptr, emo, training, seed, do_adam, lr, clip, step, stream);
}

// mmda_misa_train_step from the encoder cache.  Everything is checked before the first launch: a refused call changes nothing.
extern "C" int mmda_misa_train_step_encoded(mmda_misa* m, const mmda_encoded_batch* eb, float* emo_out, int training, uint64_t seed,
                                            int do_adam, float lr, float clip, int step, void* stream) {
  if (check_ready(m) || !m->G || !encoded_batch_ok(m, eb) || !eb->tab_emo || !emo_out) return MMDA_EINVAL;
  if (!encoder_cut(m)) return MMDA_EINVAL;               // utt would need a gradient path that nobody computes
  return train_step(m, nullptr, nullptr, nullptr, nullptr, eb, emo_out, emo_out, training, seed, do_adam, lr, clip, step, stream);
}

// The encoder cache's collect launch (encoded.hip) on the model's own workspace: B columns of the last forward of the current carve.
extern "C" int mmda_misa_encoded_collect(mmda_misa* m, float* tab_t, float* tab_v, float* tab_a, const int32_t* dst, int64_t base,
                                         void* stream) {
  if (!m || !m->ws || m->lay.B <= 0) return MMDA_EINVAL;
  // (a table that is not given is a segment that is skipped: its source is left out with it)
  return mmda_encoded_collect(tab_t ? WS(m->lay.mod[0].utt) : nullptr, tab_v ? WS(m->lay.mod[1].utt) : nullptr, tab_a ? WS(m->lay.mod[2].utt) : nullptr,
                              4 * m->par.mod[0].H, 4 * m->par.mod[1].H, 4 * m->par.mod[2].H, tab_t, tab_v, tab_a, dst, base, m->lay.B, stream);
}

// The inference pass's collect launch (infer.hip) on the model's own workspace: the sources are where the last forward of the current
// (B, T) carve left them, in the layouts that launch's comment states.
extern "C" int mmda_misa_infer_collect(mmda_misa* m, const mmda_infer_out* out, const int32_t* dst, int64_t base, void* stream) {
  if (!m || !out || !m->ws || m->lay.B <= 0) return MMDA_EINVAL;
  const Workspace& w = m->lay;
  mmda_infer_src src = {};
  src.scores = WS(w.scores); src.labels = WS(w.labels); src.tcp = WS(w.tcp); src.hfused = WS(w.hfused); src.x6 = WS(w.x6);
  src.probs = WS(w.probs);
  src.ncls = m->cfg.ncls; src.hs = m->cfg.hidden; src.nhead = NHEAD;
  return mmda_infer_collect(&src, out, dst, base, w.B, stream);
}
