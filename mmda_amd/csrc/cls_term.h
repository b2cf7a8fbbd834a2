// Internal (not part of the C ABI): the classification criterion, one element at a time.  THE arithmetic of the class-weighted / focal
// form: cls_kernel and role 0 of misc_losses_kernel (losses.hip) and the seed the forward stretch stores (fused_rows.hip) all call
// cls_term, so the three cannot drift apart.
//   lp = max(log s, -100), lq = max(log1p(-s), -100)                                   (torch's BCELoss clamp)
//   l(s, y)  = -( w_c y (1-s)^g lp + (1-y) s^g lq )
//   dl/ds    = - w_c y ( (1-s)^g / max(s, 1e-12) - g (1-s)^(g-1) lp ) + (1-y) ( s^g / max(1-s, 1e-12) - g s^(g-1) lq )
// g = 0 or 1 <= g <= 8 (mmda_cls_opts_valid): between 0 and 1, (1-s)^(g-1) diverges where lp vanishes.  Finite at s = 0 and s = 1.
// The plain criterion (no weights, g = 0) is NOT computed here: each site keeps its own expression under `cls_plain`, a launch-uniform
// branch, so the default step's bits are what they were.
#pragma once
#include "../../include/mmda_hip.h"

constexpr int CLS_MAXW = 16;              // = EVAL_MAXC (losses.hip): classes a weight list can have

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
