// Native runtime for one MISA training iteration (reference loop body solver.py:139-186 over models.py:163-285).
// Host-side C++ only: holds the parameter table, the workspace carve and the step's plan (step_plan.h makes all three), and issues the
// HIP kernels of gemm.hip / lstm.hip / norm.hip / embed_rows.hip / attn.hip / losses.hip / optim.hip in dependency order on one
// stream.  No device memory is owned here; no torch types; no host<->device synchronisation anywhere in a step.
// Five files, one concern each, over one handle (misa_handle.h; misa_pass.h: a pass and its GEMM shorthands).  This one: the handle's
// lifecycle, binding and workspace, every setter, frozen parameters, the plan's input.  misa_streams.hip: the side and background
// streams and every device resource.  misa_forward.hip, misa_backward.hip: the stages of the two passes.  misa_step.hip: losses,
// optimizer, training step.
#include "misa_handle.h"

using namespace mmda_step;
using namespace misa_rt;

namespace {

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
  m->set_mut().runs.swap(runs);
  m->set_mut().prefix_frozen = prefix_frozen; m->set_mut().embed_flag = embed_flag; m->set_mut().enc_frozen = enc_frozen;
  m->rd.runs_dirty = 1;
  return MMDA_OK;
}

// abort words of the CURRENT exchange regions -> abort_sticky (synchronous device->host copies)
int harvest_abort(mmda_misa* m) {
  if (!m->ws || !m->xc.xchg_ws || m->xc.xchg_ws != m->ws) return MMDA_OK;
  for (int i = 0; i < 3; ++i) {
    if (m->lay.mod[i].xchg < 0) continue;
    unsigned w = 0;
    if (hipMemcpy(&w, m->ws + m->lay.mod[i].xchg, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return MMDA_ELAUNCH;
    if (w) m->xc.abort_sticky = 1;
  }
  return MMDA_OK;
}

}  // namespace

namespace misa_rt {

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
  in.use_side = m->set.use_side != 0; in.use_cluster = m->set.use_cluster != 0; in.use_bf16_gemm = m->set.use_bf16_gemm != 0;
  in.inference = m->set.inference != 0; in.fusion_fp8 = m->set.fusion_fp8 != 0;
  in.embed_update = m->set.embed_update; in.embed_deferred = m->set.embed_update == EU_DENSE && m->set.df_row_step != nullptr;
  in.masked = masked(m); in.encoder_cut = encoder_cut(m); in.cut_keep_stash = m->set.cut_keep_stash != 0;
  in.bg_on = m->set.bg_on; in.bg_wgs = m->set.bg_wgs; in.moments = m->M1 && m->V1;
  in.fused = r.fused; in.has_labels = r.emo != nullptr; in.has_opt = r.opt != nullptr; in.enc_cached = r.enc_cached;
  return in;
}

}  // namespace misa_rt

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
  m->sd.release_events();
  m->bgp.release();
  m->sd.release();
  m->rd.release();
  m->tm.release();
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

extern "C" int mmda_misa_set_workspace_async(mmda_misa* m, float* ws, int64_t floats, int B, int T, void* stream) {
  if (!m || !ws || B <= 0 || T <= 0 || ((uintptr_t)ws & 15)) return MMDA_EINVAL;
  const Workspace w = carve(m->cfg, m->par, B, T);
  if (floats < w.floats) return MMDA_EINVAL;
  // The exchange regions keep their place and their contents while the buffer and B stay the same (a new T only): nothing to clear,
  // the flags there are monotonic epochs.  Otherwise they start from zero -- after the abort words of the old ones were looked at
  // (same buffer, new B: one synchronous read per region, rare; a NEW buffer: the caller reads mmda_misa_cluster_status first).
  const bool keep = m->xc.xchg_ws == ws && m->xc.xchg_B == B;
  if (!keep && m->xc.xchg_ws == ws) { int rc = harvest_abort(m); if (rc) return rc; }
  m->rebind(w);
  m->ws = ws;
  hipStream_t s = (hipStream_t)stream;
  if (!keep) {
    for (int i = 0; i < 3; ++i)
      if (w.mod[i].xchg >= 0 && hipMemsetAsync(ws + w.mod[i].xchg, 0, sizeof(float) * w.mod[i].xchg_floats, s) != hipSuccess) return MMDA_ELAUNCH;
    m->xc.xchg_ws = ws; m->xc.xchg_B = B;
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
  m->set_mut().use_side = side_stream ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_recurrence(mmda_misa* m, int resident_weights) {
  if (!m) return MMDA_EINVAL;
  m->set_mut().use_cluster = resident_weights ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_gemm_operands(mmda_misa* m, int bf16_copies) {
  if (!m) return MMDA_EINVAL;
  m->set_mut().use_bf16_gemm = bf16_copies ? 1 : 0;
  return MMDA_OK;
}
extern "C" int64_t mmda_misa_early_grad_floats(const mmda_misa* m) {
  return (m && m->st.early_valid) ? m->st.early_floats : 0;
}
extern "C" int mmda_misa_wait_early_grads(mmda_misa* m, void* stream) {
  if (!m || !m->st.early_valid || !m->sd.ev_early) return MMDA_EINVAL;
  if (hipStreamWaitEvent((hipStream_t)stream, m->sd.ev_early, 0) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_external_batch_losses(mmda_misa* m, int on) {
  if (!m) return MMDA_EINVAL;
  m->set_mut().ext_batch_losses = on ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_set_inference(mmda_misa* m, int forward_only) {
  if (!m) return MMDA_EINVAL;
  m->set_mut().inference = forward_only ? 1 : 0;
  return MMDA_OK;
}
extern "C" int mmda_misa_cluster_status(const mmda_misa* m, int* aborted_host) {
  // reads the sticky abort words of the three exchange buffers (device->host copy: call it off the step path)
  if (!m || !m->ws || !aborted_host) return MMDA_EINVAL;
  *aborted_host = m->xc.abort_sticky;          // seen in an exchange region that has since been cleared (B changed)
  if (m->sd.jflags) {                          // a flag join timed out (see SideStream::jflags)
    unsigned w = 0;
    if (hipMemcpy(&w, m->sd.jflags + 2, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return MMDA_ELAUNCH;
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

extern "C" int mmda_misa_set_adam(mmda_misa* m, const mmda_adam_opts* opts, float clip_norm) {
  if (!m || !(clip_norm >= 0.f)) return MMDA_EINVAL;
  const mmda_adam_opts o = opts ? *opts : kAdamDefaults;
  if (!mmda_adam_opts_valid(&o)) return MMDA_EINVAL;
  // deferred table: the updates that stale rows are still to replay were made with the old betas and eps
  const bool moved = o.beta1 != m->set.adam.beta1 || o.beta2 != m->set.adam.beta2 || o.eps != m->set.adam.eps;
  if (moved && m->set.df_row_step && m->df.df_flushed != m->df.df_seq) return MMDA_EINVAL;
  m->set_mut().adam = o; m->set_mut().adam.scale_dev = nullptr;
  m->set_mut().clip_norm = clip_norm;
  return MMDA_OK;
}

extern "C" int mmda_misa_set_cls_loss(mmda_misa* m, const mmda_cls_opts* opts) {
  if (!m || !mmda_cls_opts_valid(opts, m->cfg.ncls)) return MMDA_EINVAL;
  const int on = opts && !(opts->n_weights == 0 && opts->focal_gamma == 0.f);
  if (on && m->set.reg != REG_NONE) return MMDA_EINVAL;      // class weights and the focal exponent belong to the classifier
  m->set_mut().cls_on = on;
  m->set_mut().cls_opts = m->set.cls_on ? *opts : mmda_cls_opts{};
  return MMDA_OK;
}

extern "C" int mmda_misa_set_task(mmda_misa* m, int task, int loss_kind) {
  if (!m || (task != MMDA_TASK_EMOTION && task != MMDA_TASK_SENTIMENT)) return MMDA_EINVAL;
  if (task == MMDA_TASK_SENTIMENT) {
    if (loss_kind != MMDA_SENTI_L1 && loss_kind != MMDA_SENTI_MSE) return MMDA_EINVAL;
    // one output column; the confidence loss's target truth * pred is defined for labels in {0, 1}
    if (m->cfg.ncls != 1 || m->cfg.use_confidNet || m->set.cls_on) return MMDA_EINVAL;
  }
  m->set_mut().reg = task == MMDA_TASK_SENTIMENT ? 1 + loss_kind : REG_NONE;
  return MMDA_OK;
}

extern "C" int mmda_misa_set_embed_update(mmda_misa* m, int mode) {
  if (!m) return MMDA_EINVAL;
  if (mode != EU_DENSE && mode != EU_SPARSE && mode != EU_FROZEN) return MMDA_EINVAL;
  if (mode != EU_DENSE) { m->set_mut().df_row_step = nullptr; m->set_mut().df_ring = nullptr; m->set_mut().df_window = 0; }     // (the caller flushed first)
  m->set_mut().embed_update = mode;
  m->st.eu.take();
  return MMDA_OK;
}

extern "C" int mmda_misa_set_embed_deferred(mmda_misa* m, int32_t* row_step, float* step_scalars, int window, void* stream) {
  if (!m) return MMDA_EINVAL;
  if (!row_step && !step_scalars) {                        // off: plain dense from the next step on (the caller flushed first)
    m->set_mut().df_row_step = nullptr; m->set_mut().df_ring = nullptr; m->set_mut().df_window = 0; m->st.eu.take();
    return MMDA_OK;
  }
  if (!row_step || !step_scalars || window < 1 || m->set.embed_update != EU_DENSE) return MMDA_EINVAL;
  const int rc = mmda_embed_deferred_reset(row_step, m->cfg.vocab, stream);
  if (rc) return rc;
  m->set_mut().df_row_step = row_step; m->set_mut().df_ring = step_scalars; m->set_mut().df_window = window; m->st.eu.take();
  m->df.df_seq = m->df.df_flushed = 0;
  return MMDA_OK;
}

extern "C" int mmda_misa_set_embed_background(mmda_misa* m, int on, int workgroups) {
  if (!m || (on != 0 && on != 1) || workgroups < 0 || workgroups > 4096) return MMDA_EINVAL;
  m->set_mut().bg_on = on; m->set_mut().bg_wgs = workgroups;
  return MMDA_OK;
}
extern "C" int mmda_misa_embed_background_active(const mmda_misa* m) { return m ? m->bgp.bg_active : MMDA_EINVAL; }

extern "C" int mmda_misa_set_fusion_fp8(mmda_misa* m, int on) {
  if (!m) return MMDA_EINVAL;
  if (on && (m->cfg.hidden % 128) != 0) return MMDA_EINVAL;
  m->set_mut().fusion_fp8 = on ? 1 : 0;
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
  for (size_t i = 0; i + 1 < m->set.runs.size(); ++i) {
    const mmda_run& r = m->set.runs[i];
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
  m->set_mut().cut_keep_stash = keep_stash ? 1 : 0;
  return MMDA_OK;
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
