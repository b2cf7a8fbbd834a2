// One pass of the step in flight (struct Pass) and the GEMM context and shorthands its stages issue their products through.
// Included by the files that define or drive stages: misa_forward.hip, misa_backward.hip, misa_step.hip.
#pragma once
#include "misa_handle.h"

namespace misa_rt {

// ---------------------------------------------------------------------------------------------- GEMM shorthands
struct Ctx {
  mmda_misa* m; void* s; int rc = 0;
  bool grouping = false; std::vector<mmda_gemm_args> pending;
  bool absent_next = false; std::vector<mmda_gemm_args> absent;   // a product the step leaves out, still counted when the group is sized
  bool deferring = false; std::vector<mmda_gemm_args> deferred;   // weight-gradient GEMMs: off the critical path, run on the side stream
};

// independent GEMMs issued between group_begin/group_end go out as ONE grouped launch
inline void group_begin(Ctx& c) { c.grouping = true; c.pending.clear(); c.absent.clear(); }
inline void group_end(Ctx& c) {
  c.grouping = false;
  if (!c.rc && !c.pending.empty())
    c.rc = mmda_gemm_grouped_sized(c.pending.data(), (int)c.pending.size(), c.absent.data(), (int)c.absent.size(), c.s);
  c.pending.clear(); c.absent.clear();
}

inline void gemm(Ctx& c, int mode, int tA, int tB, int M, int N, int K, const float* A, int lda, const float* Bp, int ldb, float* C,
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

// y(M,N) = x(M,K) W(N,K)^T + b
inline void lin_fwd(Ctx& c, int mode, int M, int N, int K, const float* x, const float* W, const float* b, float* y, int act = 0) {
  gemm(c, mode, 0, 1, M, N, K, x, K, W, K, y, N, b, nullptr, 0, act);
}
// dx(M,K) (+)= dy(M,N) W(N,K)
inline void lin_dx(Ctx& c, int mode, int M, int N, int K, const float* dy, const float* W, float* dx, int acc) {
  gemm(c, mode, 0, 0, M, K, N, dy, N, W, K, dx, K, nullptr, nullptr, acc);
}
// dW(N,K) += dy(M,N)^T x(M,K);  db(N) += colsum(dy)
inline void lin_dw(Ctx& c, int mode, int M, int N, int K, const float* dy, const float* x, float* dW, float* db) {
  mmda_gemm_args e = {};
  e.bias_grad = db;                 // the bias gradient rides along as a virtual ones-column of the same GEMM
  gemm(c, mode, 1, 0, N, K, M, dy, N, x, K, dW, K, nullptr, nullptr, 1, 0, 1, 0, 0, 0, 0, &e);
}

// ---- row-skinny forms (fusion block at B <= SKINNY_MAX_B): see gemm_skinny.hip
// y(M,N) = act(x(M,K) W(N,K)^T + b)
inline mmda_skinny_args sk_nt(int M, int N, int K, const float* x, int ldx, const float* W, const float* b, float* y, int ldy, int act = 0) {
  mmda_skinny_args g = {};
  g.M = M; g.N = N; g.K = K; g.transB = 1; g.A = x; g.lda = ldx; g.B = W; g.ldb = K; g.C = y; g.ldc = ldy; g.bias = b; g.act = act;
  return g;
}
// dx(M,K) (+)= dy(M,N) W(N,K)
inline mmda_skinny_args sk_nn(int M, int N, int K, const float* dy, int lddy, const float* W, float* dx, int lddx, int acc) {
  mmda_skinny_args g = {};
  g.M = M; g.N = K; g.K = N; g.transB = 0; g.A = dy; g.lda = lddy; g.B = W; g.ldb = K; g.C = dx; g.ldc = lddx; g.accumulate = acc;
  return g;
}
// dx(M,K) (+)= dy(M,N) W(N,K) through the K-major copy WT(K,N): an NT problem (float4 loads along the reduction for both operands)
inline mmda_skinny_args sk_dx(int M, int N, int K, const float* dy, int lddy, const float* WT, float* dx, int lddx, int acc) {
  mmda_skinny_args g = {};
  g.M = M; g.N = K; g.K = N; g.transB = 1; g.A = dy; g.lda = lddy; g.B = WT; g.ldb = N; g.C = dx; g.ldc = lddx; g.accumulate = acc;
  return g;
}
// ... through WT where this step made the K-major copy (wt), else through W as it lies
inline mmda_skinny_args sk_dxw(bool wt, int M, int N, int K, const float* dy, int lddy, const float* WT, const float* W, float* dx, int lddx,
                        int acc) {
  return wt ? sk_dx(M, N, K, dy, lddy, WT, dx, lddx, acc) : sk_nn(M, N, K, dy, lddy, W, dx, lddx, acc);
}
inline void sk_launch(Ctx& c, const mmda_skinny_args* p, int n) {
  if (!c.rc) c.rc = mmda_gemm_skinny(p, n, c.s);
}

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
      : Ctx{m_, s_}, P(m_->st.plan), c(m_->cfg), p(m_->par), w(m_->lay), B(w.B), T(w.T), R(w.T * w.B), hs(c.hidden), NC(6 + c.ncls), mode(c.mode),
        BH((int64_t)B * hs), p_tf(m_->st.training ? c.fusion_dropout : 0.f), p_cls(m_->st.training ? c.dropout : 0.f), seed(m_->st.seed), emo(emo_), opt(opt_) {}
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

}  // namespace misa_rt
