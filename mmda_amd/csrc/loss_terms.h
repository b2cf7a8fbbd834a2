// Internal (not part of the C ABI): the element-level terms of the heads and the small losses -- one device function per term, the same
// arithmetic order and dropout indices at every site (rowlocal.h does the same for LayerNorm and attention).  The stand-alone kernels
// and the roles of misc_losses_kernel (losses.hip) and the fused stretches (fused_rows.hip) all call these, so they cannot drift apart.
// The classification criterion, one element at a time:
//   lp = max(log s, -100), lq = max(log1p(-s), -100)                                   (torch's BCELoss clamp)
//   plain (bce_plain)      l = -( y lp + (1-y) lq ),   dl/ds = (s - y) / max(s (1-s), 1e-12)      (torch binary_cross_entropy_backward)
//   weighted / focal (cls_term)
//     l(s, y)  = -( w_c y (1-s)^g lp + (1-y) s^g lq )
//     dl/ds    = - w_c y ( (1-s)^g / max(s, 1e-12) - g (1-s)^(g-1) lp ) + (1-y) ( s^g / max(1-s, 1e-12) - g s^(g-1) lq )
// g = 0 or 1 <= g <= 8 (mmda_cls_opts_valid): between 0 and 1, (1-s)^(g-1) diverges where lp vanishes.  Finite at s = 0 and s = 1.
// The plain criterion (no weights, g = 0) is computed here too, once: each site takes `cls_plain`, a launch-uniform branch, between
// bce_plain and cls_term, so the default step's bits are what they were.
// The sentiment task (mmda_misa_set_task) replaces the class head by a regression output and the criterion by reg_term:
//   head   s = z * dropout (no sigmoid: the reference's classifier is Linear, Dropout, Sigmoid and the task drops the last stage)
//   l1     l = |s - y|,    dl/ds = sign(s - y), 0 where s == y                                     (torch l1_loss backward)
//   mse    l = (s - y)^2,  dl/ds = 2 (s - y)
// both a mean over the batch.  `reg` below is REG_NONE for the classifier, else the criterion: launch-uniform wherever it is a value, a
// kernel instance of its own wherever the file has one for the weighted criterion.
#pragma once
#include "common.h"

constexpr int REG_NONE = 0, REG_L1 = 1, REG_MSE = 2;      // = 0, 1 + MMDA_SENTI_L1, 1 + MMDA_SENTI_MSE (mmda_hip.h)
__host__ __device__ __forceinline__ bool reg_valid(int reg) { return reg >= REG_NONE && reg <= REG_MSE; }

constexpr int CLS_MAXW = 16;              // = EVAL_MAXC (eval_terms.h): classes a weight list can have

// by value in the kernel arguments: no buffer, no upload
struct ClsTerm {
  float g = 0.f;                          // focusing exponent
  int nw = 0;                             // 0: every weight is 1; else the number of classes
  float w[CLS_MAXW] = {};                 // positive-class weights
};

// from the C ABI's struct (o == nullptr: plain); the caller validated it
inline ClsTerm cls_term_of(const mmda_cls_opts* o) {
  ClsTerm t;
  if (!o) return t;
  t.g = o->focal_gamma; t.nw = o->n_weights;
  for (int c = 0; c < CLS_MAXW; ++c) t.w[c] = c < o->n_weights ? o->pos_weight[c] : 0.f;
  return t;
}

__host__ __device__ __forceinline__ bool cls_plain(const ClsTerm& t) { return t.nw == 0 && t.g == 0.f; }

// value and d(value)/ds of one element of class c
__device__ __forceinline__ void cls_term(const ClsTerm& t, float s, float y, int c, float& value, float& dvalue) {
  const float lp = fmaxf(logf(s), -100.f), lq = fmaxf(log1pf(-s), -100.f);
  const float w = t.nw ? t.w[c] : 1.f;
  const float q = 1.f - s;
  float fp = 1.f, fq = 1.f, gp = 0.f, gq = 0.f;                 // (1-s)^g, s^g, g (1-s)^(g-1), g s^(g-1)
  if (t.g != 0.f) {                                             // launch-uniform (g >= 1: the exponents below are >= 0, pow(0, 0) = 1)
    fp = powf(q, t.g); fq = powf(s, t.g);
    gp = t.g * powf(q, t.g - 1.f); gq = t.g * powf(s, t.g - 1.f);
  }
  value = -(w * y * fp * lp + (1.f - y) * fq * lq);
  dvalue = -w * y * (fp / fmaxf(s, 1e-12f) - gp * lp) + (1.f - y) * (fq / fmaxf(q, 1e-12f) - gq * lq);
}

// the plain criterion: value and scale * d(value)/ds.  The scale multiplies the numerator BEFORE the division, as mmda_loss_cls always
// did; the sites that seed the step pass 1, which is exact.  (A caller that wants the gradient alone ignores `value`: the logarithms go.)
__device__ __forceinline__ void bce_plain(float s, float y, float scale, float& value, float& dvalue) {
  const float lp = fmaxf(logf(s), -100.f), lq = fmaxf(log1pf(-s), -100.f);
  value = -(y * lp + (1.f - y) * lq);
  dvalue = scale * (s - y) / fmaxf(s * (1.f - s), 1e-12f);
}

// the regression criterion: value and d(value)/ds of one element (reg: REG_L1 or REG_MSE)
__device__ __forceinline__ void reg_term(int reg, float s, float y, float& value, float& dvalue) {
  const float d = s - y;
  if (reg == REG_L1) { value = fabsf(d); dvalue = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f; }
  else { value = d * d; dvalue = 2.f * d; }
}

// the reconstruction MSE's gradient seed of one element: d = recon - orig, inv_n = 1 / elements
__device__ __forceinline__ float recon_seed(float d, float inv_n, float scale) { return 2.f * d * inv_n * scale; }

// One logit z of sample b, column c of the (B, 6 + ncls) head output: tcp = sigmoid for the six confidence columns; for class k = c - 6
// the score through the class-score dropout (element index b ncls + k) and the label against the threshold; then(k, score) follows a
// class score where it was made (the forward stretch stores the classification loss's seed there).
// H: HeadFwdArgs, or the forward stretch's own argument block, which carries the same members and is read in place.
// REG: the sentiment task's output -- the same element without the sigmoid.
struct HeadFwdArgs { int ncls; float threshold; float* tcp; float* scores; float* labels; float p_cls; uint64_t seed; int site_cls; };
template <bool REG = false, typename H, typename Then>
__device__ __forceinline__ void head_fwd_one(float z, int b, int c, const H& h, Then&& then) {
  if (c < 6) {
    h.tcp[b * 6 + c] = sigmoidf_(z);
  } else {
    const int k = c - 6;
    const float zd = z * drop_mul(h.p_cls, h.seed, h.site_cls, (uint64_t)(b * h.ncls + k));
    float s;
    if constexpr (REG) s = zd; else s = sigmoidf_(zd);
    h.scores[b * h.ncls + k] = s;
    h.labels[b * h.ncls + k] = s > h.threshold ? 1.f : 0.f;
    then(k, s);
  }
}

// d(loss)/d(logit) of the same element: sigmoid' (and the dropout multiplier of the class scores); a head without a gradient gives 0.
// REG: no s (1 - s) factor behind the regression output.
template <bool REG = false>
__device__ __forceinline__ float head_bwd_one(int b, int c, int ncls, const float* tcp, const float* scores, const float* dtcp,
                                              const float* dscores, float p, uint64_t seed, int site) {
  float g = 0.f;
  if (c < 6) {
    if (dtcp) { const float t = tcp[b * 6 + c]; g = dtcp[b * 6 + c] * t * (1.f - t); }
  } else {
    const int k = c - 6;
    if (dscores) {
      if constexpr (REG) {
        g = dscores[b * ncls + k] * drop_mul(p, seed, site, (uint64_t)(b * ncls + k));
      } else {
        const float s = scores[b * ncls + k];
        g = dscores[b * ncls + k] * s * (1.f - s) * drop_mul(p, seed, site, (uint64_t)(b * ncls + k));
      }
    }
  }
  return g;
}
