// Internal (not part of the C ABI): the figures of the evaluation reports -- one device body per figure, every launch calls it, as
// loss_terms.h does for the training losses.  A new report takes its figures from here, so two reports of the same decisions or the
// same ranking cannot differ in a bit.
// The arithmetic, stated once:
//   counts are integers (below 2^53 wherever they become doubles), every figure is float64;
//   a / b is ONE IEEE division of two integers, 0 where b <= 0 (eval_div; utils/eval.py: _div);
//   every product and every sum is rounded on its own -- no fused multiply-add -- because the host restatements (numpy:
//   metrics_from_counts, figures_from_counts) round that way: the bodies carry a function-scope `fp contract(off)`;
//   classes are added in class order, elements thread-strided and then by a fixed tree (RankFigures::reduce);
//   r / max(u, 1) with u <= EVAL_MAXC is the integer r (EVAL_LCM / u) over EVAL_LCM, so a mean of such terms is an integer sum and one
//   division.
#pragma once
#include "common.h"

constexpr int EVAL_MAXC = 16;                          // classes of a label table: 16 predicted and 16 true bits, one class lane each
constexpr unsigned long long EVAL_LCM = 720720ull;     // lcm(1 .. EVAL_MAXC)
constexpr bool eval_lcm_divides(int c) { return c > EVAL_MAXC || (EVAL_LCM % (unsigned long long)c == 0 && eval_lcm_divides(c + 1)); }
static_assert(eval_lcm_divides(1), "every c <= EVAL_MAXC divides EVAL_LCM");

__device__ __forceinline__ double eval_div(double a, double b) { return b > 0.0 ? a / b : 0.0; }

// ---- the decision figures: utils/eval.py's metrics_from_counts from per-class tp / fp / fn (the ten KEYS of get_metrics)
struct DecisionFigures {
  double f1s = 0.0, ps = 0.0, rs = 0.0, wf = 0.0, wp = 0.0, wr = 0.0, TP = 0.0, FP = 0.0, FN = 0.0;
  // the next class: its counts and the support of all classes (sum of tp + fn); hands back the class's own three figures
  __device__ __forceinline__ void add(double tp, double fp, double fn, double sup_sum, double& f1, double& prec, double& rec) {
#pragma clang fp contract(off)
    prec = eval_div(tp, tp + fp); rec = eval_div(tp, tp + fn); f1 = eval_div(2.0 * tp, 2.0 * tp + fp + fn);
    const double w = eval_div(tp + fn, sup_sum);
    f1s = f1s + f1; ps = ps + prec; rs = rs + rec;
    wf = wf + w * f1; wp = wp + w * prec; wr = wr + w * rec;
    TP = TP + tp; FP = FP + fp; FN = FN + fn;
  }
  // the ten figures of C classes.  acc = acc_num / (EVAL_LCM n) with acc_num = sum over the rows of EVAL_LCM |y & p| / max(|y | p|, 1)
  // (0 where n == 0); have_acc == false: NaN.  EVAL_LCM n is exact: n < 2^33.
  __device__ __forceinline__ void write(int C, bool have_acc, unsigned long long acc_num, unsigned long long n, double* row) const {
#pragma clang fp contract(off)
    row[0] = have_acc ? eval_div((double)acc_num, (double)(EVAL_LCM * n)) : __builtin_nan("");
    row[1] = f1s / (double)C; row[2] = ps / (double)C; row[3] = rs / (double)C;
    row[4] = eval_div(2.0 * TP, 2.0 * TP + FP + FN); row[5] = eval_div(TP, TP + FP); row[6] = eval_div(TP, TP + FN);
    row[7] = wf; row[8] = wp; row[9] = wr;
  }
};

// ---- the ranking figures of one class (ranking.py: figures_from_counts): AUROC, AP, the AP of the negatives under the negated score
// and the FPR at a TPR level, over elements of integer weight w.  An element is described by the weight of the positives / negatives
// ranked above it (gp, gn) and above or tied with it, itself included (gpep, gnen); P, Nn: the weight of all positives / negatives.
template <int WAVES>
struct RankFigures {
  unsigned long long num = 0ull, fmin = ~0ull, need;
  double ap = 0.0, apn = 0.0;
  // need: the weight of positives that makes the TPR level (at least one)
  __device__ __forceinline__ RankFigures(double level, unsigned long long P) {
    const double need_d = ceil(level * (double)P);
    need = need_d < 1.0 ? 1ull : (unsigned long long)need_d;
  }
  __device__ __forceinline__ void positive(unsigned long long w, unsigned long long gpep, unsigned long long gn, unsigned long long gnen,
                                           unsigned long long Nn) {
#pragma clang fp contract(off)
    num += w * (2ull * (Nn - gnen) + (gnen - gn));                 // twice the negatives below, once the tied ones
    ap = ap + (double)w * ((double)gpep / (double)(gpep + gnen));  // gpep >= 1: the element itself
    if (gpep >= need && gnen < fmin) fmin = gnen;
  }
  __device__ __forceinline__ void negative(unsigned long long w, unsigned long long gp, unsigned long long gn, unsigned long long P,
                                           unsigned long long Nn) {
#pragma clang fp contract(off)
    const unsigned long long lnen = Nn - gn, lpep = P - gp;        // at or below the element, itself included: lnen >= 1
    apn = apn + (double)w * ((double)lnen / (double)(lnen + lpep));
  }
  // The workgroup's totals: the xor butterfly inside a wave (the same bits in every lane: each step combines the same two numbers on
  // both sides), then thread 0 adds the waves in wave order -- a fixed tree for the two fp64 sums.  Every thread calls it, with four
  // LDS arrays of WAVES words; true in thread 0, which holds the totals.
  __device__ __forceinline__ bool reduce(unsigned long long* num_s, unsigned long long* min_s, double* ap_s, double* apn_s) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      num += __shfl_xor(num, o);
      const unsigned long long other = __shfl_xor(fmin, o);
      fmin = other < fmin ? other : fmin;
      ap += __shfl_xor(ap, o);
      apn += __shfl_xor(apn, o);
    }
    if (lane == 0) { num_s[wave] = num; min_s[wave] = fmin; ap_s[wave] = ap; apn_s[wave] = apn; }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    for (int w = 1; w < WAVES; ++w) {
      num += num_s[w];
      fmin = min_s[w] < fmin ? min_s[w] : fmin;
      ap += ap_s[w];
      apn += apn_s[w];
    }
    return true;
  }
  // n_pos, n_neg, auroc, ap, ap_neg, fpr_at_tpr; NaN where a figure needs a kind of element the class has none of
  __device__ __forceinline__ void write(unsigned long long P, unsigned long long Nn, double* row) const {
    const double nan = __builtin_nan("");
    const bool both = P > 0 && Nn > 0;
    row[0] = (double)P;
    row[1] = (double)Nn;
    row[2] = both ? (double)num / (double)(2ull * P * Nn) : nan;
    row[3] = P > 0 ? ap / (double)P : nan;
    row[4] = Nn > 0 ? apn / (double)Nn : nan;
    row[5] = both ? (double)fmin / (double)Nn : nan;               // level <= 1: need <= P, the lowest positive qualifies
  }
};

// Row C of a (C + 1, 6) ranking table, by one thread behind the class rows: per figure the mean over the classes where it is defined,
// added in class order; the first two columns count the classes that entered auroc and ap.
__device__ __forceinline__ void rank_macro_row(int C, double* tab) {
  double* macro = tab + (int64_t)C * 6;
  for (int f = 2; f < 6; ++f) {
    double sum = 0.0;
    int cnt = 0;
    for (int c = 0; c < C; ++c) {
      const double v = tab[(int64_t)c * 6 + f];
      if (v == v) { sum += v; ++cnt; }
    }
    macro[f] = cnt > 0 ? sum / (double)cnt : __builtin_nan("");
    if (f < 4) macro[f - 2] = (double)cnt;
  }
}

// ---- float64 sums without an atomic: the workgroups leave partials, and the last one to arrive -- a ticket that is 0 between
// launches -- adds them in workgroup order.  True in every thread of that workgroup, which sees every partial (release by the fence
// before the ticket, agent-scope reads after it).  Called by every thread of every workgroup; flag_s: one int of LDS.
__device__ __forceinline__ bool last_to_arrive(unsigned long long* ticket, int* flag_s) {
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long prev = atomicAdd(ticket, 1ull);
    *flag_s = prev == (unsigned long long)gridDim.x - 1ull;
  }
  __syncthreads();
  if (!*flag_s) return false;
  __threadfence();
  return true;
}
