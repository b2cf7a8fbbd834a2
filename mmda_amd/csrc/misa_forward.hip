// The forward pass of the native runtime (misa.hip): operands, the two encoder layers, the fusion block in its two forms, the side
// stream's loss chain -- from a batch or from the encoder cache.
#include "misa_pass.h"

using namespace mmda_step;
using namespace misa_rt;

namespace misa_rt {

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

// K-major (transposed) fp32 copies of the fusion block's weights for its input-gradient GEMMs in the backward pass; issued on a side
// stream that the end of forward() joins
static void weight_transpose_jobs(mmda_misa* m, std::vector<mmda_transpose_job>& tj) {
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
static int weight_transposes(mmda_misa* m, void* ss) {
  std::vector<mmda_transpose_job> tj;
  weight_transpose_jobs(m, tj);
  const int rc = mmda_transpose_f32(tj.data(), (int)tj.size(), ss);
  m->st.wT_valid = rc ? 0 : 1;
  m->st.wT_pending = 0;
  return rc;
}


// side stream, right after x6 = [private x3, shared x3] exists: clear the loss sums and the loss-seeded activation gradients,
// then DiffLoss and CMD with their gradients (they read x6 only), then the gradient bucket if train_step left that to forward()
static int eager_side_losses(mmda_misa* m, void* stream) {
  const StepPlan& P = m->st.plan;
  if (!P.fused) return MMDA_OK;
  const mmda_misa_config& c = m->cfg; const Workspace& w = m->lay;
  const int B = w.B, hs = c.hidden;
  const int64_t BH = (int64_t)B * hs;
  void* ss = nullptr;
  int rc = side_fork(m, stream, &ss);
  // (large batches: the loss chain on the side stream is the longer one by far -- the weight transposes go to the main stream)
  if (!rc && m->st.wT_pending) rc = weight_transposes(m, B >= 128 ? stream : ss);
  // (the forward stretches on the main stream STORE the seeds they own: clearing those here would race with them)
  const int64_t zend = P.seed_cls ? w.zero_cls : P.seed_recon ? w.zero_recon : w.zero_end;
  // The gradient bucket (43 MB, 11 us) is cleared on the MAIN stream behind the fork: since the row-local stretches were fused the
  // side stream's loss chain (72 us at B=32), not the main stream's fusion block (55 us), is what the join at the end of forward() waits
  // for.  (Nothing on either stream touches the bucket before the backward pass; MMDA_ZERO_GRAD_SIDE=1: the old place.)
  // ... unless the main stream will not wait for this chain before the LayerNorm-1 stretch of the backward pass (flag join on the
  // device, small batches: see SideStream::jflags) -- the chain then has two launches of slack and the clear comes back here, in ONE
  // launch with the activation-gradient region, at the head of the chain.
  if (!rc && P.zg_here && m->st.zero_grad_pending) {
    rc = mmda_zero2(WS(w.zero_begin), zend - w.zero_begin, m->G, grad_floats(m), ss);
    m->st.zero_grad_pending = 0;
  } else if (!rc) {
    if (hipMemsetAsync(WS(w.zero_begin), 0, sizeof(float) * (zend - w.zero_begin), (hipStream_t)ss) != hipSuccess) rc = MMDA_ELAUNCH;
  }
  float* L = WS(w.losses);
  if (!rc) rc = mmda_loss_diff(WS(w.x6), BH, B, hs, c.diff_weight, L + 1, WS(w.d_x6), WS(w.diff_work), ss);
  // the chain's last launch sets the flag-join word itself where it can (single-workgroup CMD: no one-thread launch behind it)
  m->st.fj1_armed = (!rc && c.use_cmd_sim && P.fj_fwd && m->sd.jflags && mmda_loss_cmd_sets_flag(B, hs)) ? 1 : 0;
  if (!rc && c.use_cmd_sim) {
    static const int sim_pairs[6] = {0, 1, 0, 2, 2, 1};      // what mmda_loss_cmd runs: (t,v), (t,a), (a,v), five moments, / 3
    rc = mmda_loss_cmd_pairs_tail(WS(w.x6 + 3 * BH), BH, 3, 3, sim_pairs, 5, B, hs, c.sim_weight, 1.0f / 3.0f, L + 2, WS(w.d_x6 + 3 * BH), ss,
                                  m->st.fj1_armed ? m->sd.jflags + 0 : nullptr, m->sd.jval[0] + 1);
  }
  if (!rc && m->st.zero_grad_pending) { rc = mmda_misa_zero_grad(m, stream); m->st.zero_grad_pending = 0; }
  m->st.eager_done = 1;
  return rc;
}

// feed-forward of the fusion transformer layer on block-scaled fp8 operands (models.py:160-161; torch's linear1 -> relu -> dropout ->
// linear2): x1 (6B, hs) -> f1 (6B, FFN) -> f2 (6B, hs).  Four launches: quantise {x1, W1, W2}, product 1 (+bias, relu, dropout),
// quantise f1, product 2 (+bias).  The f32 tensors f1 / f2 the backward pass reads are written as on the exact path.
static int ffn_fp8(mmda_misa* m, float p_tf, uint64_t seed, void* stream) {
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

// LayerNorm arguments of the fusion block: the projections' (+ activation), norm1 and norm2 (residual and dropout ride along)
mmda_ln_args Pass::proj_ln_fwd(int i) {
  mmda_ln_args ln = {};
  ln.rows = B; ln.n = hs; ln.x = WS(w.z + i * BH); ln.gamma = PP(p.mod[i].plw); ln.beta = PP(p.mod[i].plb);
  ln.y = WS(w.orig + i * BH); ln.mean = WS(w.pmean + i * B); ln.rstd = WS(w.prstd + i * B); ln.act = c.act;
  ln.eps = 1e-5f; ln.actp = act_params(m, m->st.training, seed, SITE_RRELU + i, false);
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
  l.actp = act_params(m, m->st.training, seed, SITE_RRELU + i, true);
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
  m->st.wT_reset(0);
  int Hs[12]; const float* Wp[12]; void* Fp[12]; void* Bp[12]; void* Cp[12];
  int k = 0;
  for (int i = 0; i < 3; ++i)
    for (int l = 0; l < 2; ++l)
      for (int d = 0; d < 2; ++d, ++k) {
        const RnnP& r = p.mod[i].rnn[l]; const RnnW& rw = w.mod[i].rnn[l];
        Hs[k] = r.H; Wp[k] = rW_hh(m, i, l, d); Fp[k] = WS(rw.pack_f[d]); Bp[k] = P.want_b ? WS(rw.pack_b[d]) : nullptr; Cp[k] = WS(rw.pack_c[d]);
      }
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
    m->st.wT_pending = (P.want_wT && tj.empty()) ? 1 : 0;
    if (!tj.empty()) m->st.wT_valid = rc ? 0 : 1;
  } else {
    void* ss = nullptr;
    rc = side_fork(m, s, &ss);
    if (!rc) rc = mmda_lstm_pack_whh_multi(mode, 12, Hs, Wp, Fp, Bp, P.want_c ? Cp : nullptr, ss);
    // the first recurrent kernel waits for the packing only, not for the transposes issued behind it
    if (!rc && ss != s && hipEventRecord(m->sd.ev_pack, (hipStream_t)ss) != hipSuccess) rc = MMDA_ELAUNCH;
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
  m->xc.epoch += (unsigned)T + 2u;
  group_end(*this);
  if (!rc && l == 0 && m->sd.side_pending && m->set.use_side) {   // packed W_hh ready (the side stream carries on with its transposes)
    if (hipStreamWaitEvent((hipStream_t)s, m->sd.ev_pack, 0) != hipSuccess) rc = MMDA_ELAUNCH;
  }
  if (rc) return;
  ev_rec(m, m->tm.ev_fwd, l, 0, s);
  rc = mmda_lstm_fwd(mode, 3, desc, B, T, lengths, s);
  ev_rec(m, m->tm.ev_fwd, l, 1, s);
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
  } else if (!P.fused && ((P.bfg && !P.enc_nostash) || m->st.zero_grad_pending || m->st.wT_pending)) {
    // side stream, beside the fusion block: the gradient bucket is cleared (train_step) and hseq^T of layer 2 is made for its
    // dW_hh.  Joined at the end of forward(), so everything the backward pass issues on either stream is ordered behind both.
    void* ss = nullptr;
    rc = side_fork(m, s, &ss);
    if (!rc && m->st.wT_pending) rc = weight_transposes(m, ss);
    if (!rc && m->st.zero_grad_pending && !P.fused) { rc = mmda_misa_zero_grad(m, ss); m->st.zero_grad_pending = 0; }
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
      const mmda_act_params ap = act_params(m, m->st.training, seed, SITE_RRELU_DISC, false);
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
  if (m->set.fusion_fp8) {
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
      f.p_cls = p_cls; f.seed = seed; f.site_cls = SITE_CLS; f.reg = m->set.reg;
      if (P.seed_cls) { f.emo = emo; f.d_scores = WS(w.d_scores); f.cls = cls_term_of(m->set.cls()); }
      rc = mmda_fused_fwd_c(&f, s);
    }
  } else {
    if (!rc) rc = mmda_layernorm_fwd(&l2, s);
    g[0] = sk_nt(B, NC, 6 * hs, WS(w.hfused), 6 * hs, PP(p.head_w), PP(p.head_b), WS(w.logits), NC);
    sk_launch(*this, g, 1);
    if (!rc)
      rc = mmda_heads_fwd_task(WS(w.logits), B, c.ncls, c.threshold, WS(w.tcp), WS(w.scores), WS(w.labels), p_cls, seed, SITE_CLS,
                                 m->set.reg != REG_NONE, s);
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
      const mmda_act_params ap = act_params(m, m->st.training, seed, SITE_RRELU_DISC, false);
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
  if (m->set.fusion_fp8) {
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
                               m->set.reg != REG_NONE, s);
}

// A forward pass from the projections on -- utt_t / utt_v / utt_a are in the workspace, from the encoders or from the encoder cache --
// and its tail: the K-major weight copies nobody has made yet, then the side stream's chain joined, on the device by the backward
// pass's stretch A (flag join) or by an event here.
static int forward_from_projections(Pass& x, void* stream) {
  mmda_misa* m = x.m;
  if (m->st.plan.skinny) x.fwd_fusion_skinny();
  else x.fwd_fusion_tiled();
  if (!x.rc && m->st.wT_pending) {                // no fork came by (the eager losses are off and nothing else was pending)
    void* ss = nullptr;
    x.rc = side_fork(m, stream, &ss);
    if (!x.rc) x.rc = weight_transposes(m, ss);
  }
  if (!x.rc && m->st.plan.fj_fwd && m->sd.side_pending && m->sd.jflags) {
    x.rc = side_flag_signal(m, 0, m->st.fj1_armed != 0);      // (see SideStream::jflags: fused_bwd_a_kernel waits for the loss chain)
    m->st.fj1 = x.rc ? 0 : 1; m->st.fj1_armed = 0;
    return x.rc;
  }
  if (m->st.fj1_armed) return MMDA_ELAUNCH;       // (the CMD launch was armed on the same condition: cannot happen)
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
  m->st.training = training; m->st.seed = seed;
  m->st.plan = plan_step(plan_input(m, req, m->lay.B, m->lay.T), step_switches());
  Pass x(m, stream, req.emo, req.opt);
  m->st.wT_reset(m->st.plan.want_wT ? 1 : 0);
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
  m->st.training = training; m->st.seed = seed;
  m->st.plan = plan_step(plan_input(m, req, m->lay.B, m->lay.T), step_switches());
  Pass x(m, stream, req.emo, req.opt);
  if (is_gru(m)) {          // GRU parameters -> four-slot layout (everything below reads the padded copies)
    mmda_gru_pad_job gj[MMDA_GRU_PAD_MAX];
    int n = gru_jobs(m, m->P, false, gj);
    x.rc = mmda_gru_pad_params(gj, n, stream);
    if (x.rc) return x.rc;
  }
  // deferred table update: the rows this batch gathers take the steps they missed first, so the gather reads what dense Adam left
  if (m->st.plan.embed_deferred) {
    if (!m->M1 || !m->V1) return MMDA_EINVAL;
    x.rc = mmda_embed_rows_catch_up(PP(m->par.embed), m->M1 + m->par.embed, m->V1 + m->par.embed, m->set.df_row_step, m->set.df_ring, m->set.df_window, t_ids,
                                    m->lay.B * m->lay.T, m->cfg.d_t, lengths, m->lay.B, m->cfg.vocab, m->set.adam.beta1, m->set.adam.beta2, m->set.adam.eps, m->df.df_seq, stream);
    if (x.rc) return x.rc;
  }
  const float* xin[3] = {WS(m->lay.mod[0].x), v, a};
  x.fwd_operands(t_ids, xin);
  for (int l = 0; l < 2 && !x.rc; ++l) x.fwd_encoder_layer(l, xin, lengths);
  if (x.rc) return x.rc;
  if (!m->tm.ev.empty()) { if (m->tm.ev_seen_f % m->set.ev_stride == 0) m->tm.ev_fwd++; m->tm.ev_seen_f++; }      // (the recurrent launches' timing)
  return forward_from_projections(x, stream);
}

}  // namespace misa_rt

extern "C" int mmda_misa_forward_encoded(mmda_misa* m, const mmda_encoded_batch* eb, int training, uint64_t seed, void* stream) {
  if (check_ready(m) || !encoded_batch_ok(m, eb)) return MMDA_EINVAL;
  // a training forward: utt would need a gradient path that nobody computes
  if (!m->set.inference && !encoder_cut(m)) return MMDA_EINVAL;
  return forward_encoded(m, StepRequest{false, nullptr, nullptr, true}, eb, nullptr, training, seed, stream);
}

extern "C" int mmda_misa_forward(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                                 int training, uint64_t seed, void* stream) {
  return forward_pass(m, StepRequest{}, t_ids, v, a, lengths, training, seed, stream);
}
