// The backward pass of the native runtime (misa.hip): the fusion block's dX chain in its three forms, its weight gradients and the
// side chain, the two encoder layers, the text rows' end -- and the two clears in front of it.
#include "misa_pass.h"

using namespace mmda_step;
using namespace misa_rt;

namespace misa_rt {

// bf16 operand copies that only the backward pass reads -- hseq of both layers (per direction for the tn weight-gradient GEMMs,
// transposed for the nt ones) and, nt only, the transposed layer-2 inputs: made on the side stream beside the fusion block.  <= 15 jobs.
static int backward_only_jobs(mmda_misa* m, mmda_convert_job* cj) {
  const ParamTable& p = m->par; const Workspace& w = m->lay;
  const int R = w.B * w.T;
  int n = 0;
  for (int i = 0; i < 3; ++i) {
    const ModP& md = p.mod[i]; const ModW& mw = w.mod[i];
    for (int l = 0; l < 2; ++l) {
      const RnnP& r = md.rnn[l]; const RnnW& rw = mw.rnn[l];
      if (m->st.plan.tn_wgrad) {
        for (int d = 0; d < 2; ++d)
          cj[n++] = mmda_convert_job{WS(mw.hseq[l]) + d * md.H, 2 * md.H, R, md.H, nullptr, WS(rw.hbp[d]), r.ldH, nullptr, 0};
      } else {
        cj[n++] = mmda_convert_job{WS(mw.hseq[l]), 2 * md.H, R, 2 * md.H, nullptr, nullptr, 0, WS(rw.hbT), w.ldR};
      }
    }
    if (!m->st.plan.tn_wgrad) cj[n++] = mmda_convert_job{WS(mw.normed), 2 * md.H, R, 2 * md.H, nullptr, nullptr, 0, WS(mw.rnn[1].xbT), w.ldR};
  }
  return n;
}

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
    if (m->st.fj1) f.d_tcp = nullptr;
    // the reconstruction term of stretch A's d_x6 chain, in workgroups of this launch (small batches: both sets fit the chip twice
    // over; MMDA_FUSED_SPLIT=0: inside stretch A as before)
    if (P.rec_hoisted) { f.d_recon = WS(w.d_recon); f.rec_wT = WS(w.rec_wT); f.rec_part = WS(w.rec_part); }
    f.p_cls = p_cls; f.seed = seed; f.site_cls = SITE_CLS; f.reg = m->set.reg; f.head_w = PP(p.head_w); f.d_hfused = WS(w.d_hfused); f.ln2 = norm2_bwd();
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
  if (m->st.fj1) {
    // Waiting workgroups hold their CU's LDS (104 KB each): with one on every CU the side stream's kernels could not start, and
    // the wait would never end -- on the device only while the stretch leaves most of the chip free (P.fj_device); otherwise the
    // event, here (two launches later than the end of the forward pass, where it used to be: the loss chain is the longer one at
    // large B)
    if (P.fj_device) { f.wait_flag = m->sd.jflags; f.wait_value = m->sd.jval[0]; f.wait_err = m->sd.jflags + 2; }
    else rc = flag_join_fallback(m, s);
    m->st.fj1 = 0;
  }
  if (!rc) rc = mmda_fused_bwd_a(&f, s);
  if (!P.enc_cut) skinny_proj_dx(true);                  // (d_utt feeds the encoders only)
}

// ... as stand-alone row-skinny launches (MMDA_ROW_FUSE=0, the adversarial discriminator, hidden != 128, or no K-major copies)
void Pass::bwd_fusion_skinny() {
  const bool wt = m->st.wT_valid != 0;                   // K-major weight copies from this step's forward (side stream, joined there)
  mmda_skinny_args g[8];
  rc = mmda_heads_bwd_task(WS(w.tcp), WS(w.scores), WS(w.d_tcp), WS(w.d_scores), B, c.ncls, WS(w.d_logits), p_cls, seed, SITE_CLS,
                           m->set.reg != REG_NONE, s);
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
      const mmda_act_params ap = act_params(m, m->st.training, seed, SITE_RRELU_DISC, true);
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
                           m->set.reg != REG_NONE, s);
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
      const mmda_act_params ap = act_params(m, m->st.training, seed, SITE_RRELU_DISC, true);
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
  if (!rc && m->st.misc_deferred) {
    // loss values of the step (the forward stretches stored every gradient seed: see StepState::misc_deferred)
    rc = mmda_loss_misc_reg(WS(w.scores), WS(w.tcp), m->st.misc_deferred, B, c.ncls, nullptr, nullptr, c.ncls == 6, 0, c.conf_weight,
                            WS(w.recon), WS(w.orig), 3 * BH, c.recon_weight, nullptr, nullptr, WS(w.losses), c.diff_weight,
                            c.sim_weight, c.recon_weight, c.conf_weight, c.use_confidNet, m->set.cls(), m->set.reg, ss);
    m->st.misc_deferred = nullptr;
  }
  if (!rc && P.skinny) rc = mmda_add(WS(w.x6), WS(w.x6 + 3 * BH), WS(w.rsum), 3 * BH, ss);
  // the sorted id list of the embedding scatter (see StepState::esort_valid); MMDA_SORT_EARLY=0: made where the scatter runs
  m->st.esort_valid = 0;
  // (sparse mode without an optimizer step behind this backward: the rows update runs later, in mmda_misa_adam_step, and sorts there)
  if (!rc && P.sort_early && !((P.embed_update == EU_SPARSE || P.embed_deferred) && !opt)) {
    rc = mmda_embed_sort_ids(t_ids, B * w.T, lengths, B, c.vocab, reinterpret_cast<unsigned*>(WS(w.esort)), ss);
    if (!rc && ss != s) rc = esort_signal(m, ss);
    m->st.esort_valid = rc ? 0 : (ss != s ? 2 : 1);
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
  // 68 us.  It runs as a trickle of a few workgroups under the forward pass instead: BgStream)
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
  m->xc.epoch += (unsigned)T + 2u;
  // the forward pass skipped the streaming backward packing because the resident-weights kernels were going to run: they must
  if (!P.want_b && !mmda_lstm_resident_applicable(mode, 3, desc, B, T, 1)) { rc = MMDA_EINVAL; return; }
  ev_rec(m, m->tm.ev_bwd, l == 1 ? 2 : 3, 0, s);
  rc = mmda_lstm_bwd(mode, 3, desc, B, T, lengths, s);
  ev_rec(m, m->tm.ev_bwd, l == 1 ? 2 : 3, 1, s);
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
  const bool dg_on_side = P.kdg && l == 1 && m->set.use_side && !tn;
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
    if (!m->sd.ev_early && hipEventCreateWithFlags(&m->sd.ev_early, hipEventDisableTiming) != hipSuccess) rc = MMDA_ELAUNCH;
    if (!rc && hipEventRecord(m->sd.ev_early, (hipStream_t)ss) != hipSuccess) rc = MMDA_ELAUNCH;
    m->st.early_floats = (l2_early && !is_gru(m) && P.bfg) ? p.rnn1_begin : p.rnn2_begin;
    m->st.early_valid = 1;
    // Single-GPU fused step: clip + Adam of that prefix right here, beside the layer-1 recurrence (nothing issued after this
    // point reads those fp32 parameters: the remaining GEMMs of a bf16 step read bf16 copies made in the forward pass, and in
    // the other modes the prefix ends in front of the recurrent layers).  The side stream is a real second stream only when
    // use_side is on; otherwise this is simply the same work in front of the recurrence.
    if (!rc && opt && m->st.early_floats > 0 && m->M1 && m->V1) {
      // (frozen parameters: over the prefix's trainable runs -- the prefix counts as stepped even where none of it trains)
      rc = bucket_adam(m, 0, m->st.early_floats, nullptr, opt->lr, opt->clip, opt->grad_scale, opt->step, kNoWait, ss);
      if (!rc) m->st.adam_early_done = m->st.early_floats;
    }
  } else {
    bwd_text_rows(t_ids, lengths);
  }
}

// The sorted id list that bwd_side_chain made for this pass, or nullptr (taken once).  Made on the side stream: its word, waited for
// by one wave in front of the launch that reads the list.
const unsigned* Pass::take_sorted() {
  if (!m->st.esort_valid) return nullptr;
  if (m->st.esort_valid == 2 && esort_wait(m, s)) rc = MMDA_ELAUNCH;
  m->st.esort_valid = 0;
  return reinterpret_cast<const unsigned*>(WS(w.esort));
}

// The text rows' end of the pass, behind layer 1: d_x_t goes where embed_update sends it.  Sparse and deferred tables take their rows update
// here, behind an optimizer step only (`opt`); otherwise the pass stops at d_x_t, the rows stay pending for mmda_misa_adam_step.
void Pass::bwd_text_rows(const int64_t* t_ids, const int32_t* lengths) {
  const float* dx = WS(w.mod[0].d_x);
  if (P.embed_update == EU_SPARSE || P.embed_deferred) {
    m->st.eu.take();
    if (!opt) { m->st.eu.set(t_ids, lengths); return; }
  }
  if (P.embed_update == EU_FROZEN) return;
  // the list, with the sorted form of it if this pass made one; embed_rows.hip picks the form the sums take
  const EmbedList list{t_ids, take_sorted(), R, c.d_t, dx, lengths, B};
  if (rc) return;
  if (P.embed_update == EU_SPARSE) {
    // SparseAdam on the rows the batch touches (common.h)
    SparseAdamArgs ad;
    rc = mmda_sparse_adam_args(&ad, PP(p.embed), m->M1 ? m->M1 + p.embed : nullptr, m->V1 ? m->V1 + p.embed : nullptr, c.vocab, opt->lr,
                               m->set.adam.beta1, m->set.adam.beta2, m->set.adam.eps, opt->clip, opt->grad_scale, opt->step);
    if (!rc) rc = mmda_embed_list_sparse_adam(ad, list, s);
  } else if (P.embed_deferred) {
    // dense Adam's step for the rows the batch touches (common.h: RowDenseAdam); every other row takes it when it is next needed
    if (!m->M1 || !m->V1) { rc = MMDA_EINVAL; return; }
    rc = deferred_apply(m, t_ids, list.sorted, lengths, opt->lr, m->set.adam.beta1, m->set.adam.beta2, m->set.adam.eps, opt->clip, opt->grad_scale,
                        opt->step, false, s);
  } else {
    // the gradient w.r.t. the embedding rows, scattered densely into embed.weight.grad (sparse=False)
    rc = mmda_embed_list_add(GG(p.embed), list, c.vocab, s);
  }
}

// The backward pass.  The batch (ids / v / a / lengths) is read only by what an encoder cut skips -- the encoder layers, the sorted id
// list, the scatter -- so a step from the encoder cache, which has no batch, passes NULLs: it must be a cut pass planned by a cached
// forward.
// opt: the optimizer step behind this pass, which it may start (nullptr: none, the pass stops at the gradients).
int backward_pass(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths, const OptStep* opt,
                  void* stream) {
  if (check_ready(m) || !m->G) return MMDA_EINVAL;
  if (m->st.plan.inf) return MMDA_EINVAL;                  // the last forward was an evaluation pass: nothing was stashed
  if ((!t_ids || !v || !a || !lengths) && !(m->st.plan.enc_cached && m->st.plan.enc_cut)) return MMDA_EINVAL;
  if (m->st.plan.enc_cached && !m->st.plan.enc_cut) return MMDA_EINVAL;      // (a cached forward that trains is a cut one: cannot happen)
  // the trainable set changed behind that forward: a cut pass computes no encoder gradient (and may have stashed nothing)
  if (m->st.plan.enc_cut && !encoder_cut(m)) return MMDA_EINVAL;
  if (masked(m) && opt) { const int rr = runs_ready(m, stream); if (rr) return rr; }
  m->st.begin_backward();
  Pass x(m, stream, nullptr, opt);
  const StepPlan& P = m->st.plan;
  // the fused stretches read the K-major weight copies this step's forward made (side stream, joined there)
  const bool row_fuse = P.row_fuse && m->st.wT_valid;
  if (m->st.fj1 && !row_fuse) { x.rc = flag_join_fallback(m, stream); m->st.fj1 = 0; if (x.rc) return x.rc; }     // (no kernel here waits on the device)
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
  if (!m->tm.ev.empty() && !P.enc_cached) { if (m->tm.ev_seen_b % m->set.ev_stride == 0) m->tm.ev_bwd++; m->tm.ev_seen_b++; }
  // every gradient is complete on `stream` when backward returns -- or, in a fused training step whose last optimizer launch can
  // wait on the device (see SideStream::jflags), when that launch completes
  // (only where every gradient the side stream computes lies in the prefix it also stepped -- the bf16 step, whose layer-2 weight
  //  gradients ran there in front of the early optimizer pass: the launch that waits READS the rest of the bucket before it waits)
  if (P.fj_on && opt && !is_gru(m) && m->sd.side_pending && m->sd.jflags && m->st.adam_early_done > 0 &&
      m->st.adam_early_done == m->par.rnn1_begin) {
    // (the background pass over the table joins here too: the word is set behind it, and the main stream pays nothing)
    x.rc = bg_join(m, m->sd.side);
    if (!x.rc) x.rc = side_flag_signal(m, 1);
    m->st.fj2 = x.rc ? 0 : 1;
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

}  // namespace misa_rt

extern "C" int mmda_misa_zero_act_grads(mmda_misa* m, void* stream) {
  if (check_ready(m)) return MMDA_EINVAL;
  if (hipMemsetAsync(WS(m->lay.zero_begin), 0, sizeof(float) * (m->lay.zero_end - m->lay.zero_begin), (hipStream_t)stream) != hipSuccess)
    return MMDA_ELAUNCH;
  return MMDA_OK;
}

extern "C" int mmda_misa_zero_grad(mmda_misa* m, void* stream) {
  if (!m || !m->G) return MMDA_EINVAL;
  if (hipMemsetAsync(m->G, 0, sizeof(float) * grad_floats(m), (hipStream_t)stream) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}

extern "C" int mmda_misa_backward(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                                  void* stream) {
  if (!t_ids || !v || !a || !lengths) return MMDA_EINVAL;
  return backward_pass(m, t_ids, v, a, lengths, nullptr, stream);
}
