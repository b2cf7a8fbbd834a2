// Evaluation counts on the device (mmda_amd/utils/eval.py: DeviceEval; calibrate.py: Thresholds): what get_metrics and
// get_accuracy are functions of, accumulated into a device state so that an evaluation pass over many batches needs one read-back.
//   mmda_eval_accumulate      per-class tp / fp / fn over (pred > 0, truth > 0) and the Jaccard-style accuracy sum of the reference's
//                             get_accuracy (utils/eval.py:14-31)
//   mmda_eval_accumulate_thr  the same with the labels made inside, scores > thr_c[c]: the comparison of heads_fwd_kernel with one
//                             threshold per class
//   mmda_label_counts         rows with an entry > 0, per class: the positives a class weight is made from
// The first two share one kernel and one state,
//   state[0..C) tp, [C..2C) fp, [2C..3C) fn, [3C] sum_i |y_i & p_i| / max(|y_i | p_i|, 1), [3C+1] samples      (doubles)
// added by floating-point atomics: exact for the counts, order-dependent in the Jaccard sum once a launch has more than one wave.
#include "internal.h"
#include "eval_terms.h"

namespace {

// What a launch is given beyond the table.  Nothing: the table holds the labels, predicted = table > 0.  One threshold per class and
// (optional) where to store the labels: the table holds scores, predicted = table > thr_c[c].
struct Cutoffs { const float* thr_c = nullptr; float* labels_out = nullptr; };

// One thread per row, grid-strided; a wave's sums widest step first, one atomic per non-zero sum and wave.  Cut: Cutoffs' members or
// nothing, in the kernel's argument list where the C entry point has them, so that each instance keeps the argument block (and the
// code) its stand-alone kernel had; a predictor struct passed by value would move `state`.  A pack that is not last cannot be
// deduced: both launches name it, eval_counts_kernel<> and eval_counts_kernel<const float* __restrict__, float* __restrict__>.
template <typename... Cut>
__global__ __launch_bounds__(256) void eval_counts_kernel(const float* __restrict__ table, const float* __restrict__ truth, int N, int C,
                                                          Cut... cut_args, double* state) {
  constexpr bool CUT = sizeof...(Cut) != 0;
  const Cutoffs cut{cut_args...};
  double tp[EVAL_MAXC], fp[EVAL_MAXC], fn[EVAL_MAXC];
  float thr[EVAL_MAXC];
#pragma unroll
  for (int c = 0; c < EVAL_MAXC; ++c) { tp[c] = 0.0; fp[c] = 0.0; fn[c] = 0.0; thr[c] = CUT && c < C ? cut.thr_c[c] : 0.f; }
  double jac = 0.0, cnt = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    int inter = 0, uni = 0;
#pragma unroll
    for (int c = 0; c < EVAL_MAXC; ++c) {
      if (c < C) {
        const bool y = truth[(int64_t)i * C + c] > 0.f, p = table[(int64_t)i * C + c] > thr[c];
        if (cut.labels_out) cut.labels_out[(int64_t)i * C + c] = p ? 1.f : 0.f;
        tp[c] += (y && p) ? 1.0 : 0.0; fp[c] += (!y && p) ? 1.0 : 0.0; fn[c] += (y && !p) ? 1.0 : 0.0;
        inter += (y && p) ? 1 : 0; uni += (y || p) ? 1 : 0;
      }
    }
    jac += (double)inter / (double)(uni > 0 ? uni : 1);
    cnt += 1.0;
  }
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int c = 0; c < EVAL_MAXC; ++c) {
    if (c < C) {
      const double a = wave_sum_widest_first(tp[c]), b = wave_sum_widest_first(fp[c]), d = wave_sum_widest_first(fn[c]);
      if (lead) { if (a != 0.0) atomicAdd(&state[c], a); if (b != 0.0) atomicAdd(&state[C + c], b); if (d != 0.0) atomicAdd(&state[2 * C + c], d); }
    }
  }
  jac = wave_sum_widest_first(jac); cnt = wave_sum_widest_first(cnt);
  if (lead && cnt != 0.0) { atomicAdd(&state[3 * C], jac); atomicAdd(&state[3 * C + 1], cnt); }
}

// counts[c] += rows of the (N, C) table with an entry > 0 in column c.  Integers from the lanes up: a wave's sum by shuffles, the
// workgroup's four through LDS, one 64-bit integer atomic per class and workgroup -- exact, and the same bits whatever the arrival order.
__global__ __launch_bounds__(256) void label_counts_kernel(const float* __restrict__ emo, int64_t N, int C, unsigned long long* counts) {
  __shared__ unsigned part[4][EVAL_MAXC];
  unsigned n[EVAL_MAXC];
#pragma unroll
  for (int c = 0; c < EVAL_MAXC; ++c) n[c] = 0u;
  // (a thread's count stays below 2^32: at most N / 256 rows each, N checked by the launcher)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < EVAL_MAXC; ++c)
      if (c < C) n[c] += emo[i * C + c] > 0.f ? 1u : 0u;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < EVAL_MAXC; ++c) {
    unsigned v = n[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);     // (spelled out: with wave_sum_widest_first the kernel's registers move)
    if (lane == 0) part[wave][c] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    const unsigned long long t = (unsigned long long)part[0][c] + part[1][c] + part[2][c] + part[3][c];
    if (t) atomicAdd(&counts[c], t);
  }
}

}  // namespace

extern "C" int mmda_eval_accumulate(const float* pred, const float* truth, int N, int C, double* state, void* stream) {
  if (!pred || !truth || !state || N < 0 || C <= 0 || C > EVAL_MAXC || ((uintptr_t)state & 7)) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  int blocks = (N + 255) / 256; if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(eval_counts_kernel<>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pred, truth, N, C, state);
  MMDA_CHECK_LAUNCH("mmda_eval_accumulate");
  return MMDA_OK;
}

extern "C" int mmda_eval_accumulate_thr(const float* scores, const float* truth, int N, int C, const float* thr_c, float* labels_out,
                                        double* state, void* stream) {
  if (!scores || !truth || !thr_c || !state || N < 0 || C <= 0 || C > EVAL_MAXC || ((uintptr_t)state & 7)) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  int blocks = (N + 255) / 256; if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL((eval_counts_kernel<const float* __restrict__, float* __restrict__>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, scores,
                     truth, N, C, thr_c, labels_out, state);
  MMDA_CHECK_LAUNCH("mmda_eval_accumulate_thr");
  return MMDA_OK;
}

extern "C" int mmda_label_counts(const float* emo, int64_t N, int C, int64_t* counts, void* stream) {
  if (!emo || !counts || N < 0 || C <= 0 || C > EVAL_MAXC || ((uintptr_t)counts & 7) || N > ((int64_t)1 << 40)) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  const int64_t b = (N + 255) / 256;
  const int blocks = (int)(b > 256 ? 256 : b);
  hipLaunchKernelGGL(label_counts_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, emo, N, C,
                     reinterpret_cast<unsigned long long*>(counts));
  MMDA_CHECK_LAUNCH("mmda_label_counts");
  return MMDA_OK;
}
