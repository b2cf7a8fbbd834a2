// The three values one MISA training step is built from, each made by a pure host function (step_plan.hip: no HIP call, no handle, no
// environment): the parameter table (build_params), the workspace carve (carve) and the step's plan (plan_step).  The handle (misa_handle.h)
// holds them and the misa*.hip files issue the launches they describe.
#pragma once
#include "common.h"
#include "fused_rows.h"
#include "internal.h"
#include <string>
#include <vector>

namespace mmda_step {

struct ParamInfo { std::string name; int64_t off; int rows, cols; };

// ---- ParamTable: what is fixed at create.  Offsets are floats into the flat parameter bucket (and its gradient / Adam twins).
struct RnnP {          // one bidirectional LSTM layer
  int D, H;
  int64_t w_ih, w_hh[2], b_ih, b_hh;     // w_ih: (8H,D) = [fwd;rev]; b_*: (8H) = [fwd;rev]
  int ldD, ldG, ldH;                     // leading dimensions of the bf16 operand copies, in bf16 elements: round_up(D | 8H | H, 8)
};
struct ModP {          // one modality: two stacked biLSTMs with a LayerNorm between, then a projection
  int D, H;
  RnnP rnn[2];
  int64_t ln_w, ln_b;                    // {t,v,a}layer_norm
  int64_t pw, pb, plw, plb;              // project_*: Linear + LayerNorm
};
struct ParamTable {    // built once by build_params(cfg); the handle holds it const
  std::vector<ParamInfo> params;
  int64_t dense = 0, flat = 0;
  int64_t rnn2_begin = 0, rnn1_begin = 0;    // bucket offsets where the layer-2 / layer-1 recurrent parameters start
  ModP mod[3];
  // fusion parameter offsets
  int64_t priv_w, priv_b, sh_w, sh_b, rec_w, rec_b, d1_w = -1, d1_b = -1, d2_w = -1, d2_b = -1, sp_w, sp_b;
  int64_t head_w, head_b, embed;
  int64_t in_w, in_b, out_w, out_b, l1_w, l1_b, l2_w, l2_b, n1_w, n1_b, n2_w, n2_b;
  int64_t prelu_a = -1;                      // config.activation = prelu: the ONE learned slope (nn.PReLU() shared by every use, models.py:30)
};
ParamTable build_params(const mmda_misa_config& c);

// ---- Workspace: what carve(cfg, params, B, T) returns.  Offsets are floats into the bound workspace buffer.
struct RnnW {
  int64_t pack_f[2], pack_b[2], pack_c[2];   // the packed W_hh (per direction)
  // bf16 operand copies for the bf16-mode GEMMs (leading dimensions: RnnP, and Workspace::ldR):
  int64_t wb, wbT;                           // W_ih (8H, ldD) and W_ih^T (D, ldG)
  int64_t xb, xbT;                           // layer input (R, ldD) and its transpose (D, ldR)
  int64_t dgb, dgbT;                         // gate gradients (R, ldG) and transpose (8H, ldR)
  int64_t hbT;                               // hseq^T (2H, ldR)
  int64_t hbp[2];                            // tn weight-gradient GEMMs: hseq of one direction as bf16 (R, ldH)
  // GRU (cfg.rnncell): the parameters / gradients in the four-slot layout (mmda_gru_pad_job); -1 for LSTM
  int64_t pw_ih = -1, pw_hh[2] = {-1, -1}, pb_ih = -1, pb_hh = -1, gw_ih = -1, gw_hh[2] = {-1, -1}, gb = -1;
};
struct ModW {
  RnnW rnn[2];
  int64_t x, gates[2], c[2], hseq[2], normed, ln_mean, ln_rstd, utt, d_utt, d_hseq1, d_normed, d_x, xchg, xchg_floats;
};
struct Workspace {
  int B = 0, T = 0, ldR = 0;                 // ldR = round_up(B * T, 8): rows of the transposed bf16 copies
  int64_t floats = 0;                        // the whole carve
  ModW mod[3];
  int64_t pub_begin = 0, pub_end = 0;        // the public outputs, contiguous
  int64_t zero_begin = 0, zero_end = 0;      // activation-gradient region that is zeroed per step
  int64_t zero_cls = 0, zero_recon = 0;      // ... its tail: d_scores from zero_cls, d_orig + d_recon from zero_recon (see loss seeds)
  int64_t gpad_begin = 0, gpad_end = 0;      // GRU: four-slot weight gradients (zeroed at set_workspace, re-zeroed by the unpad kernel)
  int64_t z, pmean, prstd, orig, x6, rsum, recon, dom_z, dom_h, dom, qkv, probs, ctx, attn_out, ln1_mean, ln1_rstd, x1, f1, f2,
      ln2_mean, ln2_rstd, hfused, logits, tcp, scores, labels, losses, diff_work, ffn_parts, pg_parts, ln_parts;
  // block-scaled fp8 operands of the feed-forward products (fusion_fp8): element bytes and scale bytes, as float offsets
  int64_t x1q, x1s, w1q, w1s, f1q, f1s, w2q, w2s;
  // K-major (transposed) fp32 copies of the fusion block's weights for its input-gradient GEMMs (made once per step)
  int64_t head_wT, l2_wT, l1_wT, out_wT, in_wT, rec_wT, priv_wT, sh_wT, d1_wT = -1, d2_wT = -1, pwT[3];
  int64_t d_scores, d_tcp, d_x6, d_orig, d_recon, d_dom, d_logits, d_hfused, d_x1, d_f2, d_f1, d_attn_out, d_ctx, d_qkv, d_z,
      d_dom_h, d_dom_z;
  int64_t gnorm = -1, gnorm_parts = -1;      // clip_norm: norm and coefficient of the last such step; the norm launch's block partials (doubles)
  int64_t esort = -1;                        // sorted (id, position) list of the step's text ids (see StepState::esort_valid)
  int64_t rec_part = -1;
};
// The workspace for (B, T) batches, as a value: sizes one (Workspace::floats) and is what a bound buffer is read through.
Workspace carve(const mmda_misa_config& c, const ParamTable& par, int B, int T);
// offset of a name mmda_misa_tensor_offset answers to (include/mmda_hip.h lists them) in a carve, -1 for any other name
int64_t tensor_offset(const Workspace& w, const char* name);

// embed_update: dense = the table's gradient is scattered into the bucket and dense Adam walks all V rows; sparse = the rows the batch
// touches take a SparseAdam update where their sums become final, nothing V-sized is read, written or cleared; frozen = the table
// takes no gradient at all (no text layer-1 dX product, no sort, no scatter).  In both new modes the gradient bucket ends at m->embed.
enum { EU_DENSE = 0, EU_SPARSE = 1, EU_FROZEN = 2 };
constexpr int FFN = 2048, NHEAD = 2, S6 = 6;
constexpr int SKINNY_MAX_B = 256;       // the fusion block runs on row-skinny GEMMs up to this batch (gemm_skinny.hip)
constexpr int FJ_DEVICE_MAX_B = 64;     // the forward flag join is waited for on the device up to this batch (Pass::bwd_fusion_fused)
// the background pass over the embedding table: on or off, and its workgroups, where nothing else says (measured: DESIGN section 4a)
constexpr int kEmbedBgDefault = 1, kEmbedBgWorkgroups = 32, kEmbedBgLds = 1024, kEmbedBgMaxB = 32;

// Every choice of a form of the training step, made once per forward pass by plan_step() and read by every part of the step.  Its input
// is built by plan_input() (misa.hip) from the handle's settings and the pass's StepRequest, and by nothing else.  What a launch's
// outcome sets or what is consumed later (wT_valid, side_pending, fj1, ...) stays in mmda_misa.
struct StepPlan {
  bool fused = false;               // the pass belongs to train_step: eager side losses, flag joins, the bucket clear ride inside it
  bool inf = false;                 // evaluation pass: no backward follows -- no stash, no copies that only the backward pass reads
  bool enc_cut = false;             // every encoder parameter is frozen (mmda_misa_set_trainable): the backward pass stops in front of the encoders
  bool enc_nostash = false;         // the encoders keep nothing for a backward pass: an evaluation pass, or a cut step (unless told to stash)
  bool enc_cached = false;          // the encoders did not run at all: utt came from the encoder cache (mmda_misa_forward_encoded)
  bool bfg = false;                 // bf16 mode with bf16 operand copies: the LSTM-sized GEMMs read them (gemm_bf16.hip)
  int gm = 0;                       // gate-minor layout of `gates` (see mmda_lstm_desc.gate_minor)
  bool kdg = false;                 // the backward recurrence writes the gate gradients as bf16, and only so
  bool tn_wgrad = false;            // the weight-gradient GEMMs read dG / inputs / hseq as they lie (tn form): no transposed copies
  bool want_b = false, want_c = false;     // W_hh packings made: for the streaming / the resident-weights backward kernels
  bool want_wT = false, wT_merge = false;  // K-major fusion-weight copies (row-skinny backward); made in the step's first launch
  bool skinny = false;              // fusion block on row-skinny GEMMs (B <= SKINNY_MAX_B), else on the tiled generic kernel
  bool row_fuse = false;            // ... as fused row-local stretches (the backward pass also needs wT_valid)
  bool ffn_fuse_fwd = false, ffn_fuse_bwd = false;   // the feed-forward pair fused (forward / backward differ: see plan_step)
  bool seed_recon = false, seed_cls = false;         // the forward stretches store these loss seeds (see StepState::misc_deferred)
  bool fj_on = false, fj_fwd = false, fj_device = false;   // flag joins; the forward one; ... waited for on the device
  bool zg_here = false;             // the gradient bucket is cleared at the head of the loss chain (eager_side_losses)
  bool rec_hoisted = false;         // stretch C's launch makes d_recon W_rec for stretch A
  bool sort_early = false;          // the embedding scatter's id list is sorted beside the layer-2 backward recurrence
  int embed_update = 0;             // EU_*: how the step treats the embedding table (mmda_misa_set_embed_update)
  bool embed_deferred = false;      // dense, with the table's update applied row by row when a row is next needed (mmda_misa_set_embed_deferred)
  // The table rows the batch does not index take the step on a low-priority stream beside the forward pass (BgStream; DESIGN section
  // 4a), by embed_bg_wgs workgroups, forked behind the step's first launch or (embed_bg_late) behind the layer-1 forward recurrence.
  bool embed_bg = false, embed_bg_late = false; int embed_bg_wgs = 0, embed_bg_lds = 0;
};

// The switches that select a form of the step (MMDA_GEMM_TN ... MMDA_EMBED_BG_LDS, in this order, which is also
// the order of mmda_misa_plan_describe's `switches`).  The defaults are the production path; step_switches() (misa.hip) reads the process's.
struct StepSwitches {
  int gemm_tn = 1, wt_merge = 1, row_fuse = 1, ffn_fuse = 1, loss_seeds = 1, flag_join = 1, zero_grad_side = -1, fused_split = 1,
      sort_early = 1, embed_bg = kEmbedBgDefault, embed_bg_wgs = 0, embed_bg_late = 0, embed_bg_lds = kEmbedBgLds;
};
static_assert(sizeof(StepSwitches) == MMDA_MISA_STEP_SWITCHES * sizeof(int), "mmda_misa_plan_describe copies its `switches` into one");

// Everything else plan_step reads: the configuration and shape, the handle's settings, and the four bits of the pass's request.
struct PlanInput {
  mmda_misa_config cfg; int B, T, H[3]; bool xchg[3];   // per modality: hidden size, an exchange region exists (mmda_lstm_xchg_bytes(H, B) > 0)
  bool use_side, use_cluster, use_bf16_gemm, inference, fusion_fp8, embed_deferred; int embed_update;   // (deferred: dense, the table bound)
  bool masked, encoder_cut, cut_keep_stash;    // frozen parameters: a run table is needed; the cut is in force; ... and stashes all the same
  int bg_on, bg_wgs; bool moments;             // mmda_misa_set_embed_background's two values; both Adam moment buffers are bound
  bool fused, has_labels, has_opt, enc_cached; // StepRequest: fused, emo != nullptr, opt != nullptr, enc_cached
};
StepPlan plan_step(const PlanInput& in, const StepSwitches& sw);

}  // namespace mmda_step
