// The values a MISA training step is built from (step_plan.h): the parameter table, the workspace carve and the step's plan.  Pure
// host code: no device call, no handle, no environment -- every function here is one of its arguments.
#include "step_plan.h"
#include <algorithm>
#include <cstring>

namespace mmda_step {
namespace {
int64_t add_param(ParamTable& t, const std::string& name, int rows, int cols) {
  ParamInfo p{name, t.flat, rows, cols};
  t.params.push_back(p);
  t.flat += (int64_t)rows * (cols > 0 ? cols : 1);
  return p.off;
}
}  // namespace

ParamTable build_params(const mmda_misa_config& c) {
  ParamTable t{};
  const int dims[3] = {c.d_t, c.d_v, c.d_a};
  const char* mn[3] = {"t", "v", "a"};
  const int hs = c.hidden;
  // Order of the dense bucket = the order in which the backward pass completes the gradients (data-parallel ranks start
  // reducing a prefix while the rest is still being computed, mmda_misa_early_grad_floats): fusion block and LayerNorms first,
  // then the layer-2 recurrent layers, then layer 1; the embedding matrix closes the bucket.
  for (int i = 0; i < 3; ++i) { ModP& md = t.mod[i]; md.D = md.H = dims[i]; }
  for (int i = 0; i < 3; ++i) {
    ModP& md = t.mod[i];
    std::string p = std::string("project_") + mn[i] + ".project_" + mn[i];
    md.pw = add_param(t, p + ".weight", hs, 4 * md.H);
    md.pb = add_param(t, p + ".bias", hs, 0);
    md.plw = add_param(t, p + "_layer_norm.weight", hs, 0);
    md.plb = add_param(t, p + "_layer_norm.bias", hs, 0);
  }
  // batched groups: three (hs,hs) weights back to back, then their three biases (uniform strides for batched GEMMs)
  t.priv_w = add_param(t, "private_t.private_t_1.weight", hs, hs);
  add_param(t, "private_v.private_v_1.weight", hs, hs);
  add_param(t, "private_a.private_a_3.weight", hs, hs);          // sic: reference models.py:95
  t.priv_b = add_param(t, "private_t.private_t_1.bias", hs, 0);
  add_param(t, "private_v.private_v_1.bias", hs, 0);
  add_param(t, "private_a.private_a_3.bias", hs, 0);
  t.sh_w = add_param(t, "shared.shared_1.weight", hs, hs);
  t.sh_b = add_param(t, "shared.shared_1.bias", hs, 0);
  t.rec_w = add_param(t, "recon_t.recon_t_1.weight", hs, hs);
  add_param(t, "recon_v.recon_v_1.weight", hs, hs);
  add_param(t, "recon_a.recon_a_1.weight", hs, hs);
  t.rec_b = add_param(t, "recon_t.recon_t_1.bias", hs, 0);
  add_param(t, "recon_v.recon_v_1.bias", hs, 0);
  add_param(t, "recon_a.recon_a_1.bias", hs, 0);
  if (!c.use_cmd_sim) {
    t.d1_w = add_param(t, "discriminator.discriminator_layer_1.weight", hs, hs);
    t.d1_b = add_param(t, "discriminator.discriminator_layer_1.bias", hs, 0);
    t.d2_w = add_param(t, "discriminator.discriminator_layer_2.weight", 3, hs);
    t.d2_b = add_param(t, "discriminator.discriminator_layer_2.bias", 3, 0);
  }
  t.sp_w = add_param(t, "sp_discriminator.sp_discriminator_layer_1.weight", 4, hs);
  t.sp_b = add_param(t, "sp_discriminator.sp_discriminator_layer_1.bias", 4, 0);
  // [confidence; classifier] adjacent -> one (6+ncls, 6hs) head GEMM
  t.head_w = add_param(t, "confidence.confidence_layer_1.weight", 6, 6 * hs);
  add_param(t, "classifier.classifier_layer.weight", c.ncls, 6 * hs);
  t.head_b = add_param(t, "confidence.confidence_layer_1.bias", 6, 0);
  add_param(t, "classifier.classifier_layer.bias", c.ncls, 0);
  for (int i = 0; i < 3; ++i) {
    t.mod[i].ln_w = add_param(t, std::string(mn[i]) + "layer_norm.weight", 2 * t.mod[i].H, 0);
    t.mod[i].ln_b = add_param(t, std::string(mn[i]) + "layer_norm.bias", 2 * t.mod[i].H, 0);
  }
  const std::string te = "transformer_encoder.layers.0.";
  t.in_w = add_param(t, te + "self_attn.in_proj_weight", 3 * hs, hs);
  t.in_b = add_param(t, te + "self_attn.in_proj_bias", 3 * hs, 0);
  t.out_w = add_param(t, te + "self_attn.out_proj.weight", hs, hs);
  t.out_b = add_param(t, te + "self_attn.out_proj.bias", hs, 0);
  t.l1_w = add_param(t, te + "linear1.weight", FFN, hs);
  t.l1_b = add_param(t, te + "linear1.bias", FFN, 0);
  t.l2_w = add_param(t, te + "linear2.weight", hs, FFN);
  t.l2_b = add_param(t, te + "linear2.bias", hs, 0);
  t.n1_w = add_param(t, te + "norm1.weight", hs, 0);
  t.n1_b = add_param(t, te + "norm1.bias", hs, 0);
  t.n2_w = add_param(t, te + "norm2.weight", hs, 0);
  t.n2_b = add_param(t, te + "norm2.bias", hs, 0);
  if (c.act == MMDA_ACT_PRELU) t.prelu_a = add_param(t, "activation.weight", 1, 0);      // last of the block: what follows is re-aligned
  for (int l = 1; l >= 0; --l) {
    t.flat = (t.flat + 3) & ~(int64_t)3;
    (l == 1 ? t.rnn2_begin : t.rnn1_begin) = t.flat;
    for (int i = 0; i < 3; ++i) {
      ModP& md = t.mod[i];
      RnnP& r = md.rnn[l];
      r.H = md.H; r.D = l == 0 ? md.D : 2 * md.H;
      r.ldD = round_up(r.D, 8); r.ldG = round_up(8 * r.H, 8); r.ldH = round_up(r.H, 8);
      const int ng = c.rnncell == MMDA_CELL_GRU ? 3 : 4;      // gate blocks per direction in the torch-layout parameters
      std::string pre = std::string(mn[i]) + "rnn" + (l == 0 ? "1" : "2") + ".";
      r.w_ih = add_param(t, pre + "weight_ih_l0", ng * r.H, r.D);
      add_param(t, pre + "weight_ih_l0_reverse", ng * r.H, r.D);
      r.w_hh[0] = add_param(t, pre + "weight_hh_l0", ng * r.H, r.H);
      r.w_hh[1] = add_param(t, pre + "weight_hh_l0_reverse", ng * r.H, r.H);
      r.b_ih = add_param(t, pre + "bias_ih_l0", ng * r.H, 0);
      add_param(t, pre + "bias_ih_l0_reverse", ng * r.H, 0);
      r.b_hh = add_param(t, pre + "bias_hh_l0", ng * r.H, 0);
      add_param(t, pre + "bias_hh_l0_reverse", ng * r.H, 0);
    }
  }
  t.flat = (t.flat + 3) & ~(int64_t)3;
  t.dense = t.flat;
  t.embed = add_param(t, "embed.weight", c.vocab, c.d_t);
  t.flat = (t.flat + 3) & ~(int64_t)3;
  return t;
}

Workspace carve(const mmda_misa_config& c, const ParamTable& par, int B, int T) {
  const int hs = c.hidden, NC = 6 + c.ncls;
  const int64_t R = (int64_t)T * B;
  int64_t cur = 0;
  auto take = [&cur](int64_t n) { int64_t o = cur; cur += (n + 3) & ~(int64_t)3; return o; };   // 16-B aligned
  Workspace w{};
  w.B = B; w.T = T; w.ldR = round_up(B * T, 8);
  for (int i = 0; i < 3; ++i) {       // exchange buffers of the recurrences first: their offsets depend on B only
    const ModP& md = par.mod[i]; ModW& mw = w.mod[i];
    mw.xchg_floats = (mmda_lstm_xchg_bytes(md.H, B) + 3) / 4;
    mw.xchg = mw.xchg_floats > 0 ? take(mw.xchg_floats) : -1;
  }
  for (int i = 0; i < 3; ++i) {
    const ModP& md = par.mod[i]; ModW& mw = w.mod[i];
    for (int l = 0; l < 2; ++l) {
      const RnnP& r = md.rnn[l]; RnnW& rw = mw.rnn[l];
      for (int d = 0; d < 2; ++d) {     // sized for the larger (fp32) packing so the mode can be switched in place
        rw.pack_f[d] = take(mmda_lstm_packed_bytes(MMDA_F32, r.H, 0) / 4);
        rw.pack_b[d] = take(mmda_lstm_packed_bytes(MMDA_F32, r.H, 1) / 4);
        rw.pack_c[d] = take(mmda_lstm_packed_bytes(MMDA_BF16, r.H, 2) / 4);
      }
    }
    for (int l = 0; l < 2; ++l) {
      const RnnP& r = md.rnn[l]; RnnW& rw = mw.rnn[l];
      rw.wb = take((int64_t)8 * r.H * r.ldD / 2); rw.wbT = take((int64_t)r.D * r.ldG / 2);
      rw.xb = take(R * r.ldD / 2); rw.xbT = take((int64_t)r.D * w.ldR / 2);
      rw.dgb = take(R * r.ldG / 2); rw.dgbT = take((int64_t)8 * r.H * w.ldR / 2);
      rw.hbT = take((int64_t)2 * r.H * w.ldR / 2);
      for (int d = 0; d < 2; ++d) rw.hbp[d] = take(R * r.ldH / 2);
    }
    if (c.rnncell == MMDA_CELL_GRU) {
      for (int l = 0; l < 2; ++l) {
        const RnnP& r = md.rnn[l]; RnnW& rw = mw.rnn[l];
        rw.pw_ih = take((int64_t)8 * r.H * r.D); rw.pw_hh[0] = take((int64_t)4 * r.H * r.H); rw.pw_hh[1] = take((int64_t)4 * r.H * r.H);
        rw.pb_ih = take(8 * r.H); rw.pb_hh = take(8 * r.H);
      }
    }
    mw.x = (i == 0) ? take(R * md.D) : -1;
    for (int l = 0; l < 2; ++l) {
      mw.gates[l] = take(R * 8 * md.H);
      mw.c[l] = take((int64_t)T * round_up(B, 4) * 2 * md.H);     // batch-minor-by-4 under the gate-minor layout: rows rounded up
      mw.hseq[l] = take(R * 2 * md.H);
    }
    mw.normed = take(R * 2 * md.H);
    mw.ln_mean = take(R);
    mw.ln_rstd = take(R);
    mw.utt = take((int64_t)B * 4 * md.H);
    mw.d_utt = take((int64_t)B * 4 * md.H);
    mw.d_hseq1 = take(R * 2 * md.H);
    mw.d_normed = take(R * 2 * md.H);
    mw.d_x = (i == 0) ? take(R * md.D) : -1;
  }
  const int64_t BH = (int64_t)B * hs;
  w.z = take(3 * BH); w.pmean = take(3 * B); w.prstd = take(3 * B);
  // public outputs (what the reference's solver reads off the module) are contiguous so the host can snapshot them at once
  w.pub_begin = cur;
  w.orig = take(3 * BH); w.x6 = take(6 * BH); w.recon = take(3 * BH); w.dom = take((int64_t)3 * B * 3);
  w.tcp = take((int64_t)B * 6); w.scores = take((int64_t)B * c.ncls); w.labels = take((int64_t)B * c.ncls);
  w.pub_end = cur;
  w.rsum = take(3 * BH); w.dom_z = take(3 * BH); w.dom_h = take(3 * BH);
  w.qkv = take(6 * BH * 3); w.probs = take((int64_t)B * NHEAD * S6 * S6); w.ctx = take(6 * BH);
  w.attn_out = take(6 * BH); w.ln1_mean = take(6 * B); w.ln1_rstd = take(6 * B); w.x1 = take(6 * BH);
  w.f1 = take((int64_t)6 * B * FFN); w.f2 = take(6 * BH); w.ln2_mean = take(6 * B); w.ln2_rstd = take(6 * B);
  w.hfused = take(6 * BH); w.logits = take((int64_t)B * NC);
  w.x1q = take(6 * BH / 4); w.x1s = take(6 * BH / 128 + 4); w.w1q = take((int64_t)FFN * hs / 4); w.w1s = take((int64_t)FFN * hs / 128 + 4);
  w.f1q = take((int64_t)6 * B * FFN / 4); w.f1s = take((int64_t)6 * B * FFN / 128 + 4);
  w.w2q = take((int64_t)hs * FFN / 4); w.w2s = take((int64_t)hs * FFN / 128 + 4);
  w.diff_work = take(mmda_loss_diff_work_floats(B, hs));
  w.ffn_parts = take((int64_t)(FFN / 32) * 6 * BH);      // partial products of the hidden-sliced feed-forward kernels (fused_rows.hip)
  w.ln_parts = take((int64_t)512 * 2 * 2 * (par.mod[0].H + par.mod[1].H + par.mod[2].H));   // <= 512 block partials of the three inter-layer LayerNorms' gamma / beta gradients (norm.hip)
  w.rec_part = take(3 * BH);                             // d_recon W_rec, made beside the backward pass's first stretch for its third (fused_rows.h)
  w.esort = take(2 * (int64_t)B * T + 64);              // sorted (id, position) list of the step's text ids (embed_rows.hip)
  w.pg_parts = take((int64_t)B * FUSED_PG_SLOTS * 2 * 128);      // per-sample LayerNorm gamma / beta gradient partials of the fused backward stretches
  w.head_wT = take((int64_t)6 * hs * NC); w.l2_wT = take((int64_t)FFN * hs); w.l1_wT = take((int64_t)hs * FFN);
  w.out_wT = take((int64_t)hs * hs); w.in_wT = take((int64_t)hs * 3 * hs); w.rec_wT = take((int64_t)3 * hs * hs);
  w.priv_wT = take((int64_t)3 * hs * hs); w.sh_wT = take((int64_t)hs * hs);
  if (!c.use_cmd_sim) { w.d1_wT = take((int64_t)hs * hs); w.d2_wT = take((int64_t)hs * 3); }
  for (int i = 0; i < 3; ++i) w.pwT[i] = take((int64_t)4 * par.mod[i].H * hs);
  w.gpad_begin = cur;
  if (c.rnncell == MMDA_CELL_GRU) {
    for (int i = 0; i < 3; ++i)
      for (int l = 0; l < 2; ++l) {
        const RnnP& r = par.mod[i].rnn[l]; RnnW& rw = w.mod[i].rnn[l];
        rw.gw_ih = take((int64_t)8 * r.H * r.D); rw.gw_hh[0] = take((int64_t)4 * r.H * r.H); rw.gw_hh[1] = take((int64_t)4 * r.H * r.H);
        rw.gb = take(8 * r.H);
      }
  }
  w.gpad_end = cur;
  // ---- the loss sums and the activation gradients seeded by the losses (zeroed every step by ONE memset, contiguous)
  w.zero_begin = cur;
  w.losses = take(8);
  w.d_tcp = take((int64_t)B * 6); w.d_x6 = take(6 * BH); w.d_dom = take((int64_t)3 * B * 3);
  w.zero_cls = cur;                       // (a step whose forward stores these seeds itself clears up to here only)
  w.d_scores = take((int64_t)B * c.ncls);
  w.zero_recon = cur;
  w.d_orig = take(3 * BH); w.d_recon = take(3 * BH);
  w.zero_end = cur;
  // ---- fully overwritten gradients
  w.d_logits = take((int64_t)B * NC); w.d_hfused = take(6 * BH); w.d_x1 = take(6 * BH); w.d_f2 = take(6 * BH);
  w.d_f1 = take((int64_t)6 * B * FFN); w.d_attn_out = take(6 * BH); w.d_ctx = take(6 * BH);
  w.d_qkv = take(6 * BH * 3); w.d_z = take(3 * BH); w.d_dom_h = take(3 * BH); w.d_dom_z = take(3 * BH);
  // ---- clip_norm: the gradient norm and its clip coefficient, and the norm launch's block partials (doubles, two floats each)
  w.gnorm = take(4); w.gnorm_parts = take(2 * mmda_grad_norm_partials(INT64_MAX));
  w.floats = cur;
  return w;
}

int64_t tensor_offset(const Workspace& ws, const char* name) {
  struct TensorName { const char* name; int64_t (*off)(const Workspace&); };
#define TENSOR(name, expr) {name, [](const Workspace& w) -> int64_t { return w.expr; }}
  static const TensorName names[] = {
      TENSOR("scores", scores), TENSOR("labels", labels), TENSOR("tcp", tcp), TENSOR("logits", logits), TENSOR("hfused", hfused),
      TENSOR("x6", x6), TENSOR("orig", orig), TENSOR("recon", recon), TENSOR("dom", dom), TENSOR("losses", losses),
      TENSOR("grad_norm", gnorm), TENSOR("utt_t", mod[0].utt), TENSOR("utt_v", mod[1].utt), TENSOR("utt_a", mod[2].utt),
      TENSOR("d_scores", d_scores), TENSOR("d_tcp", d_tcp), TENSOR("d_x6", d_x6), TENSOR("d_orig", d_orig), TENSOR("d_recon", d_recon),
      TENSOR("d_dom", d_dom), TENSOR("pub_begin", pub_begin), TENSOR("pub_end", pub_end), TENSOR("zero_begin", zero_begin),
      TENSOR("zero_end", zero_end), TENSOR("hseq1_t", mod[0].hseq[0]), TENSOR("hseq1_v", mod[1].hseq[0]), TENSOR("hseq1_a", mod[2].hseq[0]),
      TENSOR("d_x_t", mod[0].d_x),      // gradient w.r.t. the gathered embedding rows (T*B, d_t): the sparse form of embed.weight.grad
      TENSOR("xchg_t", mod[0].xchg), TENSOR("xchg_v", mod[1].xchg), TENSOR("xchg_a", mod[2].xchg)};   // word 0 of each = its abort word
#undef TENSOR
  for (const TensorName& t : names)
    if (!strcmp(t.name, name)) return t.off(ws);
  return -1;
}

namespace {
// Would the resident recurrences run the three layer-1 encoders (backward: 0 forward, 1 backward, 2 backward with the gate gradients
// written as bf16)?  The descriptors carry only what the resident launch plan reads -- H, cell, gate_minor and whether the exchange
// region and the resident packing exist; `present` stands for a pointer that is there and is never followed.  Asks no device.
bool probe_resident(const PlanInput& in, int gate_minor, int backward) {
  static char present;
  const int mode = in.cfg.mode;
  if (in.T <= 0 || mode != MMDA_BF16) return false;
  mmda_lstm_desc probe[3] = {};
  for (int i = 0; i < 3; ++i) {
    probe[i].H = in.H[i]; probe[i].cell = in.cfg.rnncell; probe[i].gate_minor = gate_minor;
    probe[i].xchg = (in.use_cluster && in.xchg[i]) ? &present : nullptr;
    probe[i].wpack_c[0] = probe[i].wpack_c[1] = &present;
  }
  if (backward == 2) return mmda_lstm_bwd_emits_dg_bf16(mode, 3, probe, in.B, in.T) != 0;      // ... and writes the gate gradients as bf16
  return mmda_lstm_resident_applicable(mode, 3, probe, in.B, in.T, backward) != 0;
}
}  // namespace

// the decisions of one step (see StepPlan)
StepPlan plan_step(const PlanInput& in, const StepSwitches& sw) {
  const mmda_misa_config& c = in.cfg;
  const int B = in.B, T = in.T, mode = c.mode;
  StepPlan P;
  P.fused = in.fused;
  P.inf = in.inference;
  P.enc_cut = !P.inf && in.encoder_cut;
  P.enc_nostash = P.inf || (P.enc_cut && !in.cut_keep_stash);
  P.enc_cached = in.enc_cached;
  P.bfg = mode == MMDA_BF16 && in.use_bf16_gemm;
  // which recurrent kernels will run (probe_resident) decides the packings of W_hh that are made and the layout of `gates`.
  // Gate-minor layout of the pre-activations / stash / gate gradients ([dir][unit][gate], 16-byte accesses in the recurrent
  // kernels): possible when the bf16 GEMMs produce and consume them (the interleave rides on the W_ih conversion and on the
  // GEMM epilogues) AND the resident-weights kernels will run, forward and backward.
  if (P.bfg && (B % 8) == 0 && T > 0) P.gm = probe_resident(in, 1, 0) && probe_resident(in, 1, 1);
  // The backward probe with the backward pass's own descriptors gives the same answer: they differ from these only in pointers
  // (pack_b, d_utt, d_hseq) and in wpack_c, which the backward pass sets because want_c holds -- bf16, resident, training -- and
  // without which probe_resident(1, 2) fails anyway (no exchange buffers without use_cluster).
  P.kdg = !P.enc_nostash && P.bfg && P.gm && probe_resident(in, 1, 2);
  // Weight gradients in the tn form of the bf16 GEMM (dW = dG^T X on row-major dG, X, hseq): the transposed copies of the inputs, of
  // hseq and of the gate gradients are not made at all (B=256: 0.33 ms of conversions per step).  Needs the gate gradients as bf16
  // from the recurrent kernel (gate-minor resident path).  Up to T*B = 4096 rows: measured (step, ms) B=32 0.759 -> 0.745, B=64 0.928 ->
  // 0.917, but B=128 1.362 -> 1.391, B=256 2.39 -> 2.55, T=500 4.06 -> 4.08 -- in isolation the tn kernel matches the nt one at K = 1600
  // and runs 15 - 20 % slower at K = 12800 (twice the LDS read instructions per k-tile), which at large batches outweighs the
  // conversions it saves.  Round 3: the LDS-DMA pipelined GEMM (gemm_bf16_dma_kernel) runs the tn form at K = 12800 as fast as the nt
  // form, so both layers take it at every size (B=256: the 0.47 ms of transposing conversions per step with it; a row limit, with or
  // without layer 1 alone in the tn form beyond it, measured slower).  MMDA_GEMM_TN=0: the transposed-copy (nt) form everywhere.
  P.tn_wgrad = P.kdg && sw.gemm_tn;
  // The forward packing always; the resident-weights backward packing when those kernels will run the backward pass and the
  // streaming backward packing only when they will not; neither for a pass whose encoders keep no stash.
  P.want_c = !P.enc_nostash && in.use_cluster && mode == MMDA_BF16;
  P.want_b = !P.enc_nostash && !(P.want_c && probe_resident(in, 0, 1));
  P.skinny = B <= SKINNY_MAX_B;
  P.want_wT = P.skinny && !P.inf;
  P.wT_merge = P.bfg && P.want_wT && sw.wt_merge;
  // The row-local stretches as one launch each (fused_rows.hip): recon + qkv -> attention -> out-proj -> LayerNorm 1, and LayerNorm 2
  // -> heads; backward: heads' sigmoid' -> d_hfused -> LayerNorm 2, and LayerNorm 1 -> ... -> the projection LayerNorms.
  // MMDA_ROW_FUSE=0: the launches they replace (4 and 3 forward, 3 and 6 backward).
  P.row_fuse = P.skinny && sw.row_fuse && c.use_cmd_sim && c.hidden == 128 && NHEAD == 2;
  // The feed-forward pair as one launch split over the hidden units.  The fp8 forward (fusion_fp8) has products of its own, but the
  // backward pass reads the f32 f1 / f2 it writes like the exact path's, so the fused dX kernel serves it as well.
  P.ffn_fuse_fwd = P.row_fuse && sw.ffn_fuse && !in.fusion_fp8 && (FFN % 32) == 0;
  P.ffn_fuse_bwd = P.row_fuse && sw.ffn_fuse && (FFN % 32) == 0;
  // loss seeds by the stretches of a fused step that knows its labels (see StepState::misc_deferred); MMDA_LOSS_SEEDS=0: by the loss
  // launch behind the forward pass, as before
  P.seed_recon = sw.loss_seeds && P.row_fuse && in.fused && in.has_labels;
  P.seed_cls = P.seed_recon && !c.use_confidNet;
  // flag joins (see SideStream::jflags) in a fused training step
  P.fj_on = sw.flag_join && in.use_side && in.fused;
  P.fj_fwd = P.fj_on && P.seed_recon && P.seed_cls;
  P.fj_device = P.fj_fwd && B <= FJ_DEVICE_MAX_B;
  P.zg_here = sw.zero_grad_side >= 0 ? sw.zero_grad_side != 0 : P.fj_device;
  P.rec_hoisted = sw.fused_split && B <= 64;
  P.embed_update = in.embed_update;
  P.embed_deferred = in.embed_deferred;
  P.sort_early = sw.sort_early && T > 0 && mmda_embed_scatter_sorts(T * B) && P.embed_update != EU_FROZEN && !P.enc_cut;
  // The background pass: a fused step from a batch with the native Adam behind it and no norm clip (has_opt: train_step), a plain
  // dense table, nothing frozen (no run table).  Not under clip_norm: a non-finite norm poisons the zero gradients of the dense launch
  // too, and that must stay so.  The table is whole quads and fewer than 2^31 floats (the walkers' index arithmetic).
  // Where it pays (measured): up to one 32-sample batch group of the resident recurrences, which then hold 152 of the
  // CUs; from the second group on they want every CU, and the pass's workgroups -- which keep off a recurrence's CUs by holding LDS --
  // delay their placement (B=64: 0.763 -> 0.816 ms).  MMDA_EMBED_BG=2, or the handle's own switch: wherever the step is eligible.
  const int bg_switch = in.bg_on >= 0 ? (in.bg_on ? 2 : 0) : sw.embed_bg;
  const int64_t tab = (int64_t)c.vocab * c.d_t;
  P.embed_bg = bg_switch != 0 && (bg_switch >= 2 || B <= kEmbedBgMaxB) && in.has_opt && !P.enc_cached && !P.enc_cut && P.embed_update == EU_DENSE &&
               !P.embed_deferred && !in.masked && T > 0 && in.moments && tab > 0 && (tab & 3) == 0 && tab < ((int64_t)1 << 31);
  P.embed_bg_late = sw.embed_bg_late != 0;
  P.embed_bg_lds = std::max(0, std::min(65536, sw.embed_bg_lds));
  P.embed_bg_wgs = std::min(4096, in.bg_wgs > 0 ? in.bg_wgs : sw.embed_bg_wgs > 0 ? sw.embed_bg_wgs : kEmbedBgWorkgroups);
  return P;
}

}  // namespace mmda_step
