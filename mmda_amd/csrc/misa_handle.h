// The model handle (struct mmda_misa) of the native runtime, shared by the misa*.hip files: two values made by step_plan.h (the
// parameter table, the workspace carve), the bound buffers, and four groups of members as types of their own, one lifetime each --
// Settings, the device resources (SideStream, BgStream, RunsDev, Timing, Xchg), the deferred table's counters and StepState.  The small
// predicates and accessors every stage calls are inline here; the functions that cross files are declared at the end.
#pragma once
#include "step_plan.h"
#include <algorithm>
#include <cstring>

namespace misa_rt {
using namespace mmda_step;

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

// The model's Adam unless mmda_misa_set_adam says otherwise (the reference gives torch.optim.Adam nothing but lr)
constexpr mmda_adam_opts kAdamDefaults = {0.9f, 0.999f, 1e-8f, 0.f, 0, nullptr};

// ---- settings, written only by mmda_misa_set_* (and mmda_misa_timing_stride / _rotate) through mmda_misa::set_mut(); every stage of
// a pass reads them through the const view mmda_misa::set
struct Settings {
  // The optimizer's settings (mmda_misa_set_adam): every Adam launch of the handle reads them; scale_dev is not kept (a step with
  // clip_norm > 0 points its launches at gnorm[1]).  clip_norm > 0: clip_grad_norm_ in front of the update -- no update may precede the
  // norm, so such a step takes no early optimizer pass.
  mmda_adam_opts adam = kAdamDefaults;
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
  int bg_on = -1, bg_wgs = 0;                // mmda_misa_set_embed_background; -1 / 0: MMDA_EMBED_BG's / MMDA_EMBED_BG_WGS's (else the default)
  // (the pass's workgroups hold LDS they never touch, MMDA_EMBED_BG_LDS bytes: a resident recurrence reserves the whole LDS of its CUs,
  //  so the two never share a CU -- sharing one cost each forward recurrence 24 us of its hand-offs at any throttle)
  int ev_stride = 1;               // record every ev_stride-th step (the event pairs cost ~35 us per step)
  int ev_rotate = 0;               // 1: a sampled step brackets ONE of the four recurrent launches (sample index % 4): ~9 us
};

// ---- device resources (created lazily, released by mmda_misa_destroy; no device memory but jflags, row_stamp and runs_dev).  Each
// type holds the counters that number its words; create() / release() are in misa_streams.hip, the only callers of HIP among them.
struct SideStream {
  hipStream_t side = nullptr;      // second stream for weight-gradient GEMMs
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_pack = nullptr;
  hipEvent_t ev_early = nullptr;             // recorded by backward() when the gradients of the bucket prefix are final
  // Flag joins (training step; common.h: flag_wait): where the main stream needs a side-stream chain's results, the consuming KERNEL
  // waits on the device for a word that a one-thread launch behind the chain sets, instead of the stream waiting for an event -- an
  // event wait costs the main stream 9 - 12 us of packet processing even when the chain finished long ago (tools/micro/fork_cost.hip),
  // twice per step.  Forward: the loss chain's gradients (d_x6) are first read by the LayerNorm-1 stretch of the backward pass
  // (fused_bwd_a_kernel).  Backward: nothing on the main stream reads what the side stream's weight-gradient GEMMs and early
  // optimizer pass write; the step's last optimizer launch simply does not complete before they have.  ev_join is still recorded
  // behind each chain for the paths that cannot wait on the device.  MMDA_FLAG_JOIN=0: event joins as before.
  unsigned* jflags = nullptr;                // device: [0] forward chain done, [1] backward chain done, [2] a wait timed out, [3] id list sorted
  unsigned jval[2] = {0u, 0u};               // the values the flag-join words [0], [1] were last set to
  unsigned esort_val = 0u;                   // ... and word [3] (StepState::esort_valid)
  int side_pending = 0;
  int create(unsigned evf);                  // the stream, its three fork / join events (flags evf) and the words, at the first fork
  void release_events();                     // mmda_misa_destroy: the four events go first, the stream and the words behind BgStream's
  void release();
};
// The background pass over the embedding table (StepPlan::embed_bg).  A row the batch does not index has gradient zero, and its Adam
// step needs nothing the step computes: a few workgroups on `bg`, a stream of the lowest priority, trickle that update under the
// forward pass, where HBM is nearly idle, and the step's closing launch walks only the rows the batch does index.  Which rows those
// are: row_stamp[V] on the device, where the launch that reads the step's ids writes bg_epoch (internal.h: RowStamp) -- padding
// positions too, so the gather never reads a row the pass writes; no clear per step, the epoch moves on (all stamps are cleared
// when it wraps to 0).  Fork: ev_bg_fork behind that launch, so the pass is ordered behind the stamps, the previous step and whatever
// the caller queued.  Join: ev_bg_done, waited for by the side stream in front of the word it sets for the closing launch (flag
// join), else by the main stream behind that launch.  All created at the first eligible step.
struct BgStream {
  hipStream_t bg = nullptr; hipEvent_t ev_bg_fork = nullptr, ev_bg_done = nullptr;
  unsigned* row_stamp = nullptr; unsigned bg_epoch = 0u;
  int bg_pending = 0, bg_active = 0;         // the pass went out and is not joined yet; the last train_step ran it
  int create(size_t stamp_bytes, unsigned evf);      // whatever of the stream, its events and the stamps is not there yet
  void release();
};
// runs_dev: the table of trainable runs on the device (the one allocation besides jflags), copied when the set has changed since
// the last launch that read it (runs_ready).
struct RunsDev {
  mmda_run* runs_dev = nullptr; int runs_dev_cap = 0; int runs_dirty = 1;
  void release();
};
// optional per-launch timing of the four recurrent kernels (bench.py roofline leg)
struct Timing {
  std::vector<hipEvent_t> ev;      // [step][slot][start/stop]
  int ev_steps = 0, ev_fwd = 0, ev_bwd = 0;
  int ev_seen_f = 0, ev_seen_b = 0;
  std::vector<char> ev_done;                         // (step, slot) was recorded
  void release();                  // destroys the events (mmda_misa_timing_end clears the rest)
};
// cluster-exchange regions: at the front of the workspace, sized by B alone, so a change of T (every batch under the reference's
// collate) neither moves nor clears them -- flags are monotonic epochs.  Cleared (on the caller's stream) only when the buffer
// or B changes; the abort words found there before a clear are kept in `abort_sticky`.
struct Xchg {
  float* xchg_ws = nullptr; int xchg_B = 0; int abort_sticky = 0;
  unsigned epoch = 1;              // monotonic cluster-exchange epoch (never reset; see lstm_resident.h)
};
// deferred table: df_seq: updates applied since the binding (what a current row's row_step equals); df_flushed: df_seq at the last full flush.
struct DeferredCount { int df_seq = 0, df_flushed = 0; };

// ---- the state of the step in flight.  A group of fields that is reset at one site is one function here, called from that site;
// wT_valid, early_valid, eu and plan outlive the call that wrote them (later, separate API calls read them).
struct StepState {
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
  // state of the last forward (dropout replay in backward)
  int training = 0; uint64_t seed = 0;
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
  // The sort-based embedding scatter of a large batch in two halves: the sorted (id, position) list depends on the ids only and is
  // made on the side stream beside the layer-2 backward recurrence (33 us of launches at B=256 that used to sit between the last
  // GEMM and the optimizer); word [3] tells the main stream it is there (a one-wave wait launch in front of the sums).
  int esort_valid = 0;
  int fj1 = 0, fj2 = 0, fj1_armed = 0;
  // train_step_body, in front of the step's first launch
  void begin_train_step(bool has_T) {
    zero_grad_pending = has_T ? 1 : 0;
    eager_done = 0; misc_deferred = nullptr;
    fj1 = fj2 = 0;
  }
  // backward_pass, behind its checks
  void begin_backward() { early_valid = 0; adam_early_done = 0; }
  // the top of a forward pass: last step's K-major copies are stale; `pending`: this step's ride on its first fork
  void wT_reset(int pending) { wT_valid = 0; wT_pending = pending; }
};

}  // namespace misa_rt

struct mmda_misa {
  explicit mmda_misa(const mmda_misa_config& c) : cfg(c), par(mmda_step::build_params(c)) {}
  mmda_misa(const mmda_misa&) = delete;      // (`lay` and `set` refer to this handle's own values)
  mmda_misa_config cfg;                      // fixed at create, but for cfg.mode (mmda_misa_set_mode)
  const mmda_step::ParamTable par;           // fixed at create
  const mmda_step::Workspace& lay = lay_;    // the carve of the bound (B, T): read-only but for ...
  void rebind(const mmda_step::Workspace& v) { lay_ = v; }   // ... mmda_misa_set_workspace_async, which replaces it as a whole
  // ---- bound buffers (mmda_misa_bind, mmda_misa_set_workspace_async)
  float *P = nullptr, *G = nullptr, *M1 = nullptr, *V1 = nullptr;
  float* ws = nullptr;
  const misa_rt::Settings& set = set_;       // what every pass reads: a stage that assigns a setting does not compile
  // ... but for the extern "C" setters and apply_trainable -- and train_step, which clears `inference`
  misa_rt::Settings& set_mut() { return set_; }
  misa_rt::SideStream sd;
  misa_rt::BgStream bgp;
  misa_rt::RunsDev rd;
  misa_rt::Timing tm;
  misa_rt::Xchg xc;
  misa_rt::DeferredCount df;                 // beside Settings::df_row_step, whose updates it counts
  misa_rt::StepState st;

 private:
  mmda_step::Workspace lay_{};
  misa_rt::Settings set_{};
};

namespace misa_rt {

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

// parameters of a parametrised activation (prelu / rrelu) at one of its uses; zeros for every other activation
inline mmda_act_params act_params(mmda_misa* m, int training, uint64_t seed, int site, bool grads) {
  mmda_act_params p = {};
  if (m->cfg.act == MMDA_ACT_PRELU) { p.slope = m->P + m->par.prelu_a; p.dslope = grads ? m->G + m->par.prelu_a : nullptr; }
  if (m->cfg.act == MMDA_ACT_RRELU) { p.lo = 1.0f / 8.0f; p.hi = 1.0f / 3.0f; p.rand = training ? 1 : 0; p.seed = seed; p.site = site; }   // torch defaults
  return p;
}

inline int check_ready(const mmda_misa* m) {
  if (!m || !m->P || !m->ws) return MMDA_EINVAL;
  return MMDA_OK;
}

// recurrent descriptor of modality i, layer l: forward (W_hh packed for the forward kernels, utt) or backward (streaming backward
// packing, the resident-weights one where `with_c`, d_utt, d(hseq of layer 1))
inline mmda_lstm_desc lstm_desc(mmda_misa* m, int i, int l, bool bwd, int gate_minor, bool with_c) {
  const ModW& mw = m->lay.mod[i]; const RnnW& rw = mw.rnn[l];
  const int64_t* wp = bwd ? rw.pack_b : rw.pack_f;
  mmda_lstm_desc d = {};
  d.H = m->par.mod[i].rnn[l].H; d.gates = WS(mw.gates[l]); d.cstash = WS(mw.c[l]); d.hseq = WS(mw.hseq[l]);
  d.wpack[0] = WS(wp[0]); d.wpack[1] = WS(wp[1]);
  if (with_c) { d.wpack_c[0] = WS(rw.pack_c[0]); d.wpack_c[1] = WS(rw.pack_c[1]); }
  d.utt = WS(bwd ? mw.d_utt : mw.utt); d.layer = l; d.d_hseq = bwd && l == 0 ? WS(mw.d_hseq1) : nullptr;
  d.xchg = (m->set.use_cluster && mw.xchg >= 0) ? (void*)WS(mw.xchg) : nullptr; d.epoch_base = m->xc.epoch;
  d.gate_minor = gate_minor; d.cell = m->cfg.rnncell;
  return d;
}

// floats of the gradient bucket that a step writes, clears and walks with dense Adam: all of it, or the prefix in front of the table
inline int64_t grad_floats(const mmda_misa* m) { return m->set.embed_update == EU_DENSE && !m->set.df_row_step ? m->par.flat : m->par.embed; }

// ---- frozen parameters
// a launch over [0, grad_floats) has a frozen float to leave out (else the step is today's: the dense kernels, the early pass)
inline bool masked(const mmda_misa* m) { return m->set.prefix_frozen || (!m->set.embed_flag && grad_floats(m) == m->par.flat); }
// the encoder cut: nothing behind the fusion block trains -- the recurrent layers and the inter-layer LayerNorms are frozen and the
// table is, by its flag (dense) or by embed_update (the sparse and deferred modes train the table through d_x: no cut)
inline bool encoder_cut(const mmda_misa* m) {
  return m->set.enc_frozen && (m->set.embed_update == EU_FROZEN || (m->set.embed_update == EU_DENSE && !m->set.df_row_step && !m->set.embed_flag));
}
// the table's slice for the bucket range [lo, hi), both of them 0, rnn2_begin, rnn1_begin, embed or flat
inline void runs_slice(const mmda_misa* m, int64_t lo, int64_t hi, int* r0, int* n, int64_t* items) {
  const int nr = (int)m->set.runs.size() - 1;
  int a = 0;
  while (a < nr && m->set.runs[a].begin < lo) ++a;
  int b = a;
  while (b < nr && m->set.runs[b].begin < hi) ++b;
  *r0 = a; *n = b - a; *items = m->set.runs[b].first - m->set.runs[a].first;
}

// the background pass's view of the table and of the step's Adam (see BgStream)
inline TableRows bg_table(const mmda_misa* m) { return TableRows{m->bgp.row_stamp, m->bgp.bg_epoch, m->cfg.vocab, m->cfg.d_t}; }
inline AdamHyper bg_hyper(const mmda_misa* m, const OptStep& o) {
  return AdamHyper{o.lr, m->set.adam.beta1, m->set.adam.beta2, m->set.adam.eps, o.clip, o.grad_scale, o.step, m->set.adam.weight_decay, m->set.adam.decoupled, nullptr};
}

// ---- the functions that cross files
// misa.hip
const StepSwitches& step_switches();
PlanInput plan_input(const mmda_misa* m, const StepRequest& r, int B, int T);
// misa_streams.hip.  Fork/join with the side stream: everything issued on the forked stream only has to be finished before the optimizer
// step, so it runs concurrently with the recurrent kernels (which occupy ~10 % of the CUs while they walk the serial chain).
int side_fork(mmda_misa* m, void* main_stream, void** out);
int side_launch(mmda_misa* m, std::vector<mmda_gemm_args>& list, void* main_stream);
int side_join(mmda_misa* m, void* main_stream);
int side_flag_signal(mmda_misa* m, int idx, bool by_kernel = false);
int flag_join_fallback(mmda_misa* m, void* main_stream);
int esort_signal(mmda_misa* m, void* side_stream);
int esort_wait(mmda_misa* m, void* main_stream);
int bg_begin(mmda_misa* m, const int64_t* ids, int n, void* main_stream, RowStamp* st);
int bg_launch(mmda_misa* m, const OptStep* opt, void* main_stream);
int bg_join(mmda_misa* m, void* stream);
int runs_ready(mmda_misa* m, void* stream);
void ev_rec(mmda_misa* m, int step, int slot, int which, void* stream);
// misa_forward.hip
int gru_jobs(mmda_misa* m, float* base, bool grads, mmda_gru_pad_job* j);
bool encoded_batch_ok(const mmda_misa* m, const mmda_encoded_batch* eb);
int forward_encoded(mmda_misa* m, const StepRequest& req, const mmda_encoded_batch* eb, float* emo_out, int training, uint64_t seed,
                    void* stream);
int forward_pass(mmda_misa* m, const StepRequest& req, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                 int training, uint64_t seed, void* stream);
// misa_backward.hip
int backward_pass(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths, const OptStep* opt,
                  void* stream);
// misa_step.hip
int bucket_adam(mmda_misa* m, int64_t lo, int64_t hi, const float* acc, float lr, float clip, float grad_scale, int step, const FlagWait& w,
                void* stream, const float* scale_dev = nullptr);
int deferred_apply(mmda_misa* m, const int64_t* ids, const unsigned* sorted, const int32_t* lengths, float lr, float beta1, float beta2,
                   float eps, float clip, float grad_scale, int step, bool catch_up, void* stream);

}  // namespace misa_rt
