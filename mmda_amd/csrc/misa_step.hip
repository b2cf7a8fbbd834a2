// Losses, the optimizer and the training step of the native runtime (misa.hip): what follows a forward pass.
#include "misa_pass.h"

using namespace mmda_step;
using namespace misa_rt;

namespace misa_rt {

// clamp + Adam over the bucket range [lo, hi) with the gradient G, or acc + G (acc != nullptr: the accumulator, laid out like the
// bucket): the dense stream, or -- frozen parameters -- the trainable runs of that range, where a range with nothing to train launches
// nothing but for a waiter (w.flag != nullptr).
// scale_dev: the clip coefficient of a step with clip_norm > 0 (bucket_norm below), else nullptr.
int bucket_adam(mmda_misa* m, int64_t lo, int64_t hi, const float* acc, float lr, float clip, float grad_scale, int step, const FlagWait& w,
                void* stream, const float* scale_dev) {
  const AdamHyper h{lr, m->set.adam.beta1, m->set.adam.beta2, m->set.adam.eps, clip, grad_scale, step, m->set.adam.weight_decay, m->set.adam.decoupled, scale_dev};
  if (!masked(m)) return mmda_adam_launch(m->P + lo, acc ? acc + lo : nullptr, m->G + lo, m->M1 + lo, m->V1 + lo, hi - lo, nullptr, h, w, stream);
  int r0 = 0, n = 0; int64_t items = 0;
  runs_slice(m, lo, hi, &r0, &n, &items);
  if (n > 0 && (m->rd.runs_dirty || !m->rd.runs_dev)) return MMDA_EINVAL;      // (every entry that gets here called runs_ready first)
  const RunTable t{n > 0 ? m->rd.runs_dev + r0 : nullptr, n, items};
  return mmda_adam_launch(m->P, acc, m->G, m->M1, m->V1, 0, &t, h, w, stream);
}
// clip_norm > 0: the norm of the gradient the step is about to apply -- G or acc + G over [0, grad_floats), the trainable runs of it
// when parameters are frozen -- and the clip coefficient, into gnorm[0], gnorm[1]
static int bucket_norm(mmda_misa* m, const float* acc, float grad_scale, void* stream) {
  if (!m->ws || m->lay.gnorm < 0) return MMDA_EINVAL;
  double* parts = reinterpret_cast<double*>(m->ws + m->lay.gnorm_parts);
  const int64_t cap = mmda_grad_norm_partials(INT64_MAX);
  const int64_t hi = grad_floats(m);
  if (!masked(m)) return mmda_grad_norm_launch(m->G, acc, hi, nullptr, m->set.clip_norm, grad_scale, parts, cap, m->ws + m->lay.gnorm, stream);
  int r0 = 0, n = 0; int64_t items = 0;
  runs_slice(m, 0, hi, &r0, &n, &items);
  if (n > 0 && (m->rd.runs_dirty || !m->rd.runs_dev)) return MMDA_EINVAL;
  const RunTable t{n > 0 ? m->rd.runs_dev + r0 : nullptr, n, items};
  return mmda_grad_norm_launch(m->G, acc, 0, &t, m->set.clip_norm, grad_scale, parts, cap, m->ws + m->lay.gnorm, stream);
}
// what no step does (checked in front of its first launch, so a refused call changes nothing): decay under the deferred table -- the
// replay ring holds two scalars per update, a decayed zero-gradient step needs a third; a norm clip with a table whose rows are updated
// where their sums become final, before a norm exists
static bool adam_settings_refused(const mmda_misa* m) {
  if (m->set.adam.weight_decay > 0.f && m->set.df_row_step) return true;
  if (m->set.clip_norm > 0.f && (m->set.embed_update == EU_SPARSE || m->set.df_row_step)) return true;
  return false;
}

// update df_seq + 1 of the deferred table for the rows of one backward's id list, counted here and nowhere else
int deferred_apply(mmda_misa* m, const int64_t* ids, const unsigned* sorted, const int32_t* lengths, float lr, float beta1, float beta2,
                   float eps, float clip, float grad_scale, int step, bool catch_up, void* stream) {
  if (!m->set.df_row_step || !m->P || !m->M1 || !m->V1 || !m->ws || m->lay.T <= 0 || !ids) return MMDA_EINVAL;
  if (m->df.df_seq == INT32_MAX) return MMDA_EINVAL;
  const int seq = m->df.df_seq + 1;
  const int rc = mmda_embed_dense_adam_apply(PP(m->par.embed), m->M1 + m->par.embed, m->V1 + m->par.embed, m->set.df_row_step, m->set.df_ring, m->set.df_window, ids,
                                             sorted, m->lay.B * m->lay.T, m->cfg.d_t, WS(m->lay.mod[0].d_x), lengths, m->lay.B, m->cfg.vocab, lr, beta1,
                                             beta2, eps, clip, grad_scale, seq, step, catch_up, stream);
  if (rc) return rc;
  if (seq % m->set.df_window == 0) m->df.df_flushed = seq - 1;    // (that update flushed first)
  m->df.df_seq = seq;
  return MMDA_OK;
}

// sparse table: the rows of the backward that just ran (d_x_t is workspace: the next micro-batch overwrites it) go to the caller's list
static int accum_append_rows(mmda_misa* m, const RowList& l, void* stream) {
  if (!m->st.eu.on || !m->ws || m->lay.T <= 0 || !l.ids || !l.rows) return MMDA_EINVAL;
  const PendingRows r = m->st.eu.take();                   // (a later mmda_misa_adam_step must not apply these rows again)
  return mmda_embed_rows_append(l.ids, l.rows, l.used, l.capacity, r.ids, WS(m->lay.mod[0].d_x), m->lay.B * m->lay.T, m->cfg.d_t, r.lengths, m->lay.B, stream);
}
static bool accum_ready(const mmda_misa* m) { return m && m->P && m->G && !m->set.df_row_step; }
// sparse table: a backward is pending and the list holds its T B rows behind the `used` it already has (dense / frozen: no list)
static bool accum_list_ok(const mmda_misa* m, const RowList& l) {
  if (m->set.embed_update != EU_SPARSE) return true;
  const int64_t R = (int64_t)m->lay.B * m->lay.T;
  return m->st.eu.on && m->ws && m->lay.T > 0 && l.ids && l.rows && l.used >= 0 && l.used <= l.capacity && R <= l.capacity - l.used &&
         l.used + R <= INT32_MAX;
}

// What every optimizer step is checked for in front of its first launch, so that a refused call changes nothing
static int opt_step_refused(const mmda_misa* m, const OptStep& o) {
  if (!m->P || !m->G || !m->M1 || !m->V1 || o.step < 1 || (o.norm && !m->ws)) return MMDA_EINVAL;
  return adam_settings_refused(m) ? MMDA_EINVAL : MMDA_OK;
}

// The optimizer part of a step, from bucket offset lo (an early pass stepped what lies in front of it): the run table where parameters
// are frozen, the norm, clamp + Adam over [lo, grad_floats) -- w: that launch waits for the side stream's word -- and the table's rows
// that are still to be updated: the accumulated step's list (sparse table), or the rows a backward left pending (sparse, deferred).
// (Behind a fused step nothing is pending: bwd_text_rows takes m->st.eu whenever it is handed a step, and a cut pass, which does not get
// that far, needs a frozen or plain dense table (encoder_cut), where the rows part does not apply.)
static int opt_step(mmda_misa* m, const OptStep& o, int64_t lo, const FlagWait& w, const RowList* list, void* stream) {
  int rc = masked(m) ? runs_ready(m, stream) : MMDA_OK;
  if (!rc && o.norm) rc = bucket_norm(m, o.acc, o.grad_scale, stream);
  if (!rc) rc = bucket_adam(m, lo, grad_floats(m), o.acc, o.lr, o.clip, o.grad_scale, o.step, w, stream, o.norm ? m->ws + m->lay.gnorm + 1 : nullptr);
  if (rc) return rc;
  float* const p = PP(m->par.embed); float* const m1 = m->M1 + m->par.embed; float* const v1 = m->V1 + m->par.embed; const mmda_adam_opts& h = m->set.adam;
  if (m->set.embed_update == EU_SPARSE && list) {
    const int n = (int)(list->used + (int64_t)m->lay.B * m->lay.T);
    rc = accum_append_rows(m, *list, stream);
    // SparseAdam on the rows any micro-batch touched, sums in list order (micro-batch major); padding went in as id -1
    if (!rc) rc = mmda_embed_rows_sparse_adam(p, m1, v1, list->ids, n, m->cfg.d_t, list->rows, nullptr, 0, m->cfg.vocab, o.lr, h.beta1, h.beta2,
                                              h.eps, o.clip, o.grad_scale, o.step, stream);
  } else if (m->set.embed_update == EU_SPARSE && m->st.eu.on) {
    // the touched rows of the last backward: coalesce, scale, clamp, SparseAdam (the clamp applies to the coalesced sum)
    const PendingRows r = m->st.eu.take();
    if (!m->ws || m->lay.T <= 0) return MMDA_EINVAL;
    rc = mmda_embed_rows_sparse_adam(p, m1, v1, r.ids, m->lay.B * m->lay.T, m->cfg.d_t, WS(m->lay.mod[0].d_x), r.lengths, m->lay.B, m->cfg.vocab, o.lr, h.beta1,
                                     h.beta2, h.eps, o.clip, o.grad_scale, o.step, stream);
  } else if (m->set.embed_update == EU_DENSE && m->set.df_row_step && m->st.eu.on) {
    rc = mmda_misa_embed_deferred_step(m, o.lr, h.beta1, h.beta2, h.eps, o.clip, o.grad_scale, o.step, stream);
  }
  return rc;
}

// One training step: from a batch (t_ids, v, a, lengths; labels `emo`), or -- eb != nullptr -- from the encoder cache, whose forward
// gathers the labels into `emo` itself.  The two differ in their forward pass and in the batch the backward pass is handed, nowhere else.
// (the body of train_step below, which closes it: whatever this returns, the background pass over the table is joined)
static int train_step_body(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths, const mmda_encoded_batch* eb,
                    float* emo_gathered, const float* emo, int training, uint64_t seed, int do_adam, float lr, float clip, int step,
                    void* stream) {
  // the gradient bucket is cleared on the side stream beside the forward pass's fusion block (not at the start of the step: the
  // side stream's first job there, packing W_hh, is what the first recurrent kernel waits for)
  if (check_ready(m) || !m->G) return MMDA_EINVAL;
  // clip_norm: no update may precede the norm, so the backward pass runs as it does without an optimizer step (no early pass, event
  // join); the norm and one launch over the whole bucket follow it
  const OptStep o{lr, clip, 1.0f, step, nullptr, do_adam && m->set.clip_norm > 0.f};
  const bool early = do_adam && !o.norm;
  int rc = do_adam ? opt_step_refused(m, o) : MMDA_OK;
  if (!rc && do_adam && masked(m)) rc = runs_ready(m, stream);     // frozen parameters: the run table is there before the first launch
  if (rc) return rc;
  m->set_mut().inference = 0;                                     // a training step always stashes (but for the encoders of a cut step)
  m->st.begin_train_step(m->lay.T > 0);
  // opt: the kind of step that may run the background pass over the table (plan_step decides): from a batch, the native Adam behind it, no norm
  const StepRequest req{true, emo, (early && !eb) ? &o : nullptr, eb != nullptr};
  rc = m->st.zero_grad_pending ? MMDA_OK : mmda_misa_zero_grad(m, stream);
  if (!rc) rc = eb ? forward_encoded(m, req, eb, emo_gathered, training, seed, stream) : forward_pass(m, req, t_ids, v, a, lengths, training, seed, stream);
  if (rc) return rc;
  if (m->st.zero_grad_pending) return MMDA_ELAUNCH;        // forward() always reaches its fusion block
  rc = mmda_misa_losses(m, emo, 1, stream);
  if (rc) return rc;
  // (the early optimizer pass beside the layer-1 recurrence: faster than one launch for the whole bucket at the end)
  rc = backward_pass(m, t_ids, v, a, lengths, early ? &o : nullptr, stream);
  if (rc) return rc;
  if (m->st.fj1) { rc = flag_join_fallback(m, stream); m->st.fj1 = 0; if (rc) return rc; }      // (no stretch took it over: cannot happen)
  if (m->st.fj2 && !early) { rc = flag_join_fallback(m, stream); m->st.fj2 = 0; if (rc) return rc; }
  if (!do_adam) return MMDA_OK;
  // the rest of the bucket (layer-1 recurrent layers, embedding -- or everything, if the backward pass stepped nothing early; a sparse
  // or frozen table: the launch ends in front of it); flag join: it does not complete before the side stream's chain has
  const bool fj = m->st.fj2 != 0;
  m->st.fj2 = 0;
  const FlagWait w = fj ? FlagWait{m->sd.jflags + 1, m->sd.jval[1], m->sd.jflags + 2} : kNoWait;
  if (!m->bgp.bg_active) return opt_step(m, o, m->st.adam_early_done, w, nullptr, stream);
  // The background pass stepped the table rows this batch does not index: the launch covers the rest of the bucket in front of the
  // table and the rows whose stamp is this step's, which read the scattered gradient -- one launch, as ever.  (Such a step has no run
  // table, no norm, no accumulator and no pending rows: plan_step.)
  const int64_t lo = m->st.adam_early_done;
  return mmda_adam_tail_launch(m->P + lo, m->G + lo, m->M1 + lo, m->V1 + lo, m->par.embed - lo, bg_table(m), bg_hyper(m, o), w, stream);
}

static int train_step(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths, const mmda_encoded_batch* eb,
               float* emo_gathered, const float* emo, int training, uint64_t seed, int do_adam, float lr, float clip, int step,
               void* stream) {
  if (m) m->bgp.bg_active = 0;
  const int rc = train_step_body(m, t_ids, v, a, lengths, eb, emo_gathered, emo, training, seed, do_adam, lr, clip, step, stream);
  // Where the side stream did not take the pass's join into its flag word (fp32 step, MMDA_FLAG_JOIN=0, GRU, no early optimizer pass,
  // a step that failed half-way), the caller's stream waits for it here, behind the closing launch.
  const int rj = (m && m->bgp.bg_pending) ? bg_join(m, stream) : MMDA_OK;
  return rc ? rc : rj;
}

}  // namespace misa_rt

extern "C" int mmda_misa_losses(mmda_misa* m, const float* emo, int with_grads, void* stream) {
  if (check_ready(m) || !emo) return MMDA_EINVAL;
  const mmda_misa_config& c = m->cfg; const Workspace& w = m->lay;
  const int B = w.B, hs = c.hidden;
  const int64_t BH = (int64_t)B * hs;
  hipStream_t s = (hipStream_t)stream;
  int rc = MMDA_OK;
  float* L = WS(w.losses);
  const bool ext = m->set.ext_batch_losses && with_grads && c.use_cmd_sim;      // the caller did (see Settings::ext_batch_losses)
  const bool eager = (m->st.eager_done || ext) && with_grads;        // forward() already cleared the region and ran diff (+ CMD) on the side stream
  // seeds the forward stretches stored already: the plan's, while this call takes up that forward pass's chain (eager_done)
  const bool s_recon = m->st.eager_done && with_grads && m->st.plan.seed_recon, s_cls = m->st.eager_done && with_grads && m->st.plan.seed_cls;
  m->st.eager_done = 0;
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
    m->st.misc_deferred = emo;
    return MMDA_OK;
  }
  return mmda_loss_misc_reg(WS(w.scores), WS(w.tcp), emo, B, c.ncls, (with_grads && !s_cls) ? WS(w.d_scores) : nullptr,
                            (with_grads && !s_cls) ? WS(w.d_tcp) : nullptr, c.ncls == 6 && !ext, with_grads && c.use_confidNet && !ext,
                            c.conf_weight, WS(w.recon), WS(w.orig), 3 * BH, c.recon_weight, (with_grads && !s_recon) ? WS(w.d_recon) : nullptr,
                            (with_grads && !s_recon) ? WS(w.d_orig) : nullptr, L, c.diff_weight, c.sim_weight, c.recon_weight, c.conf_weight,
                            c.use_confidNet, m->set.cls(), m->set.reg, stream);
}

extern "C" int mmda_misa_embed_flush(mmda_misa* m, void* stream) {
  if (!m) return MMDA_EINVAL;
  if (!m->set.df_row_step) return MMDA_OK;                     // nothing is deferred
  if (!m->P || !m->M1 || !m->V1) return MMDA_EINVAL;
  if (m->df.df_flushed == m->df.df_seq) return MMDA_OK;          // no update since the last flush: nothing is stale, nothing is launched
  const int rc = mmda_embed_rows_flush(PP(m->par.embed), m->M1 + m->par.embed, m->V1 + m->par.embed, m->set.df_row_step, m->set.df_ring, m->set.df_window,
                                       m->cfg.d_t, m->cfg.vocab, m->set.adam.beta1, m->set.adam.beta2, m->set.adam.eps, m->df.df_seq, stream);
  if (!rc) m->df.df_flushed = m->df.df_seq;
  return rc;
}

extern "C" int mmda_misa_embed_deferred_step(mmda_misa* m, float lr, float beta1, float beta2, float eps, float clip, float grad_scale,
                                             int step, void* stream) {
  if (!m || !m->set.df_row_step || m->set.embed_update != EU_DENSE || !m->st.eu.on || step < 1) return MMDA_EINVAL;
  const PendingRows r = m->st.eu.take();
  // (another forward may have run since that backward: its rows are brought to the last update again, which costs one launch)
  return deferred_apply(m, r.ids, nullptr, r.lengths, lr, beta1, beta2, eps, clip, grad_scale, step, true, stream);
}

extern "C" int mmda_misa_adam_step(mmda_misa* m, float lr, float clip, float grad_scale, int step, void* stream) {
  if (!m) return MMDA_EINVAL;
  const OptStep o{lr, clip, grad_scale, step, nullptr, m->set.clip_norm > 0.f};
  const int rc = opt_step_refused(m, o);
  return rc ? rc : opt_step(m, o, 0, kNoWait, nullptr, stream);
}

// ---- accumulated steps (accum_steps > 1): the micro-batch is mmda_misa_train_step(do_adam = 0); what happens to its gradients is here
extern "C" int mmda_misa_grad_accumulate(mmda_misa* m, float* acc, int first, int64_t* list_ids, float* list_rows, int64_t list_used,
                                         int64_t list_capacity, void* stream) {
  const RowList l{list_ids, list_rows, list_used, list_capacity};
  if (!accum_ready(m) || !acc || !accum_list_ok(m, l)) return MMDA_EINVAL;
  int rc = mmda_grad_accumulate(acc, m->G, grad_floats(m), first, stream);
  if (!rc && m->set.embed_update == EU_SPARSE) rc = accum_append_rows(m, l, stream);
  return rc;
}

extern "C" int mmda_misa_adam_step_accumulated(mmda_misa* m, const float* acc, int64_t* list_ids, float* list_rows, int64_t list_used,
                                               int64_t list_capacity, float lr, float clip, float grad_scale, int step, void* stream) {
  const RowList l{list_ids, list_rows, list_used, list_capacity};
  if (!accum_ready(m) || !accum_list_ok(m, l)) return MMDA_EINVAL;
  const OptStep o{lr, clip, grad_scale, step, acc, m->set.clip_norm > 0.f};
  const int rc = opt_step_refused(m, o);
  return rc ? rc : opt_step(m, o, 0, kNoWait, &l, stream);
}

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
