// Threshold calibration on the device (mmda_amd/calibrate.py: ThresholdSweep, Thresholds).  The model decides
// labels = scores > threshold (reference models.py:249, functions.py:112-115; heads_fwd_kernel's fp32 `s > thr`) and everything the
// reference's evaluation reports moves with that cut-off.  Three entry points:
//   mmda_calib_accumulate     every cut-off of a grid at once: per class a histogram of score bins split by truth, and per cut-off the
//                             (|y & p|, |y | p|) pair counts of the rows -- all that get_metrics / get_accuracy are functions of
//   mmda_calib_select         one workgroup: the ten figures at every cut-off and the arg max of one of them, written on the device
//   mmda_eval_accumulate_thr  mmda_eval_accumulate with the labels made inside from one threshold per class
// The sweep counts in integers only (32-bit LDS atomics per workgroup, 64-bit global adds of the non-zero bins), so its result does not
// depend on the order of arrival: two runs give the same bits.  Sweep and selection use no floating-point atomic; the third entry
// point keeps mmda_eval_accumulate's state of doubles and its adds (exact for tp / fp / fn, order-dependent in the Jaccard sum).
#include "internal.h"

namespace {

constexpr int CALIB_MAXC = 16;                // = EVAL_MAXC (losses.hip)
constexpr int CALIB_MAXK = 256;
constexpr int CALIB_ROWS = 32;                // rows of one workgroup tile
constexpr int CALIB_GRID_CAP = 256;           // workgroups along the rows; beyond it a workgroup strides
// One workgroup counts EITHER the histogram (blockIdx.y == 0: C (K + 1) 2 words, at most 16 * 257 * 2) OR the pair table of one chunk
// of thresholds (blockIdx.y - 1: kc (C + 1)^2 words, kc sized on the host to fit), so one array serves both: 32.1 KB, with the grid 33.1.
constexpr int CALIB_WORDS = CALIB_MAXC * (CALIB_MAXK + 1) * 2;

// bin(s) = #{k : s > thr[k]} for a strictly increasing grid: the first k with !(s > thr[k]).  A NaN is greater than nothing: bin 0.
__device__ __forceinline__ int calib_bin(float s, const float* thr_s, int K) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s > thr_s[mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// blockIdx.x: a tile of CALIB_ROWS rows, then on by gridDim.x tiles.  blockIdx.y == 0: one thread per (row, class) element, a binary
// search in the LDS copy of the grid and one LDS add.  blockIdx.y >= 1: one thread per (row, threshold of the chunk) with the threshold
// running fastest, so a wave's LDS adds go to different tables (stride (C + 1)^2 words) and its loads of a row are one address.
// n_rows < 2^31 per launch (host), so no 32-bit count can wrap.
__global__ __launch_bounds__(256) void calib_accumulate_kernel(const float* __restrict__ scores, const float* __restrict__ truth,
                                                               int64_t N, int C, const float* __restrict__ thr, int K, int kc,
                                                               unsigned long long* __restrict__ hist,
                                                               unsigned long long* __restrict__ pairs) {
  __shared__ float thr_s[CALIB_MAXK];
  __shared__ unsigned cnt_s[CALIB_WORDS];
  const int tid = threadIdx.x;
  const bool do_hist = blockIdx.y == 0;
  const int P = (C + 1) * (C + 1);
  const int k0 = do_hist ? 0 : ((int)blockIdx.y - 1) * kc;
  const int kn = do_hist ? 0 : min(kc, K - k0);                 // thresholds of this chunk
  const int words = do_hist ? C * (K + 1) * 2 : kn * P;
  for (int i = tid; i < K; i += 256) thr_s[i] = thr[i];
  for (int i = tid; i < words; i += 256) cnt_s[i] = 0u;
  __syncthreads();
  for (int64_t r0 = (int64_t)blockIdx.x * CALIB_ROWS; r0 < N; r0 += (int64_t)gridDim.x * CALIB_ROWS) {
    const int rows = (int)min((int64_t)CALIB_ROWS, N - r0);
    if (do_hist) {
      for (int it = tid; it < rows * C; it += 256) {
        const int64_t e = r0 * C + it;
        const int c = it % C;
        const int bin = calib_bin(scores[e], thr_s, K);
        atomicAdd(&cnt_s[(c * (K + 1) + bin) * 2 + (truth[e] > 0.f ? 1 : 0)], 1u);
      }
    } else {
      for (int it = tid; it < rows * kn; it += 256) {
        const int row = it / kn, kk = it - row * kn;
        const float t = thr_s[k0 + kk];
        const float* s = scores + (r0 + row) * C;
        const float* y = truth + (r0 + row) * C;
        int a = 0, b = 0;
        for (int c = 0; c < C; ++c) {
          const bool p = s[c] > t, q = y[c] > 0.f;
          a += (p && q) ? 1 : 0; b += (p || q) ? 1 : 0;
        }
        atomicAdd(&cnt_s[kk * P + a * (C + 1) + b], 1u);
      }
    }
  }
  __syncthreads();
  unsigned long long* out = do_hist ? hist : pairs + (int64_t)k0 * P;
  for (int i = tid; i < words; i += 256) {
    const unsigned v = cnt_s[i];
    if (v) atomicAdd(&out[i], (unsigned long long)v);
  }
}

// ------------------------------------------------------------------------------------------------ select
// zero where the denominator is zero (utils/eval.py: _div); both operands are integers below 2^53, so the quotient is one IEEE division
__device__ __forceinline__ double calib_div(double a, double b) { return b > 0.0 ? a / b : 0.0; }

// arg max over v[0 .. K) by one wave, ties to the lowest index; the same value in every lane
__device__ __forceinline__ int wave_argmax_first(const double* v, int K, int lane) {
  double best = -1.0; int at = 0x7fffffff;                      // every figure is >= 0
  for (int k = lane; k < K; k += WAVE)
    if (v[k] > best) { best = v[k]; at = k; }
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const double ob = __shfl_xor(best, o);
    const int oa = __shfl_xor(at, o);
    if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
  }
  return at;
}

constexpr unsigned long long CALIB_LCM = 720720ull;             // lcm(1 .. 16): a / max(b, 1) as an integer multiple of 1 / 720720

// One workgroup of 256 threads, thread k = cut-off k.  Per class: tp[k] = sum_{j > k} hist[c][j][1], fp[k] likewise from [0], by an
// integer suffix scan in LDS; fn from the class's positive total.  All arithmetic fp64, classes added in index order.
__global__ __launch_bounds__(256) void calib_select_kernel(const unsigned long long* __restrict__ hist,
                                                           const unsigned long long* __restrict__ pairs, int C, int K,
                                                           const float* __restrict__ thr, int col, int per_class,
                                                           float* __restrict__ out_thr, int32_t* __restrict__ out_k,
                                                           double* __restrict__ table) {
  __shared__ unsigned long long scan_s[2][CALIB_MAXK];
  __shared__ unsigned long long tot_s[CALIB_MAXC][2];
  __shared__ double f1_s[CALIB_MAXC][CALIB_MAXK];              // per-class F1 at every cut-off: what per_class selects on
  __shared__ double obj_s[CALIB_MAXK];
  const int k = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = k < K;
  if (k < 2 * C) {                                              // class totals: [c][0] negatives, [c][1] positives
    const int c = k >> 1, p = k & 1;
    unsigned long long t = 0;
    for (int j = 0; j <= K; ++j) t += hist[((int64_t)c * (K + 1) + j) * 2 + p];
    tot_s[c][p] = t;
  }
  __syncthreads();
  unsigned long long sup_all = 0;
  for (int c = 0; c < C; ++c) sup_all += tot_s[c][1];
  const unsigned long long n_rows = tot_s[0][0] + tot_s[0][1];
  unsigned long long TP = 0, FP = 0, FN = 0;
  double f1_sum = 0.0, p_sum = 0.0, r_sum = 0.0, wf1 = 0.0, wp = 0.0, wr = 0.0;
  for (int c = 0; c < C; ++c) {
    if (live) {
      scan_s[0][k] = hist[((int64_t)c * (K + 1) + k + 1) * 2];
      scan_s[1][k] = hist[((int64_t)c * (K + 1) + k + 1) * 2 + 1];
    }
    __syncthreads();
    for (int o = 1; o < K; o <<= 1) {
      unsigned long long a0 = 0, a1 = 0;
      if (live && k + o < K) { a0 = scan_s[0][k + o]; a1 = scan_s[1][k + o]; }
      __syncthreads();
      if (live) { scan_s[0][k] += a0; scan_s[1][k] += a1; }
      __syncthreads();
    }
    if (live) {
      const unsigned long long tpi = scan_s[1][k], fpi = scan_s[0][k], fni = tot_s[c][1] - tpi;
      const double tp = (double)tpi, fp = (double)fpi, fn = (double)fni;
      const double prec = calib_div(tp, tp + fp), rec = calib_div(tp, tp + fn), f1 = calib_div(2.0 * tp, 2.0 * tp + fp + fn);
      const double w = calib_div((double)tot_s[c][1], (double)sup_all);
      f1_sum += f1; p_sum += prec; r_sum += rec;
      wf1 += w * f1; wp += w * prec; wr += w * rec;
      TP += tpi; FP += fpi; FN += fni;
      f1_s[c][k] = f1;
    }
    __syncthreads();                                            // scan_s is loaded again
  }
  if (live) {
    double row[10];
    if (pairs) {
      unsigned long long num = 0;
      const unsigned long long* pk = pairs + (int64_t)k * (C + 1) * (C + 1);
      for (int a = 1; a <= C; ++a)
        for (int b = a; b <= C; ++b)                            // |y & p| <= |y | p|: the other entries are zero
          num += pk[a * (C + 1) + b] * (unsigned long long)a * (CALIB_LCM / (unsigned long long)b);
      row[0] = calib_div((double)num, (double)(CALIB_LCM * n_rows));
    } else {
      row[0] = __builtin_nan("");
    }
    const double tp = (double)TP, fp = (double)FP, fn = (double)FN;
    row[1] = f1_sum / (double)C; row[2] = p_sum / (double)C; row[3] = r_sum / (double)C;
    row[4] = calib_div(2.0 * tp, 2.0 * tp + fp + fn); row[5] = calib_div(tp, tp + fp); row[6] = calib_div(tp, tp + fn);
    row[7] = wf1; row[8] = wp; row[9] = wr;
    if (table)
      for (int i = 0; i < 10; ++i) table[(int64_t)k * 10 + i] = row[i];
    obj_s[k] = row[col];
  }
  __syncthreads();
  if (per_class) {
    for (int c = wave; c < C; c += 4) {
      const int at = wave_argmax_first(f1_s[c], K, lane);
      if (lane == 0) { out_k[c] = at; out_thr[c] = thr[at]; }
    }
  } else if (wave == 0) {
    const int at = wave_argmax_first(obj_s, K, lane);
    if (lane < C) { out_k[lane] = at; out_thr[lane] = thr[at]; }
  }
}

// ------------------------------------------------------------------------------------------------ evaluation counts from scores
// eval_counts_kernel (losses.hip) with the prediction made here: p = scores > thr_c[c], the comparison of heads_fwd_kernel with one
// threshold per class.  The same state, the same order of the per-thread and per-wave sums.
__global__ __launch_bounds__(256) void eval_counts_thr_kernel(const float* __restrict__ scores, const float* __restrict__ truth, int N,
                                                              int C, const float* __restrict__ thr_c, float* __restrict__ labels_out,
                                                              double* state) {
  double tp[CALIB_MAXC], fp[CALIB_MAXC], fn[CALIB_MAXC];
  float thr[CALIB_MAXC];
#pragma unroll
  for (int c = 0; c < CALIB_MAXC; ++c) { tp[c] = 0.0; fp[c] = 0.0; fn[c] = 0.0; thr[c] = c < C ? thr_c[c] : 0.f; }
  double jac = 0.0, cnt = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    int inter = 0, uni = 0;
#pragma unroll
    for (int c = 0; c < CALIB_MAXC; ++c) {
      if (c < C) {
        const bool y = truth[(int64_t)i * C + c] > 0.f, p = scores[(int64_t)i * C + c] > thr[c];
        if (labels_out) labels_out[(int64_t)i * C + c] = p ? 1.f : 0.f;
        tp[c] += (y && p) ? 1.0 : 0.0; fp[c] += (!y && p) ? 1.0 : 0.0; fn[c] += (y && !p) ? 1.0 : 0.0;
        inter += (y && p) ? 1 : 0; uni += (y || p) ? 1 : 0;
      }
    }
    jac += (double)inter / (double)(uni > 0 ? uni : 1);
    cnt += 1.0;
  }
  auto wsum = [](double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
  };
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int c = 0; c < CALIB_MAXC; ++c) {
    if (c < C) {
      const double a = wsum(tp[c]), b = wsum(fp[c]), d = wsum(fn[c]);
      if (lead) { if (a != 0.0) atomicAdd(&state[c], a); if (b != 0.0) atomicAdd(&state[C + c], b); if (d != 0.0) atomicAdd(&state[2 * C + c], d); }
    }
  }
  jac = wsum(jac); cnt = wsum(cnt);
  if (lead && cnt != 0.0) { atomicAdd(&state[3 * C], jac); atomicAdd(&state[3 * C + 1], cnt); }
}

}  // namespace

extern "C" int mmda_calib_accumulate(const float* scores, const float* truth, int64_t N, int C, const float* thr, int K,
                                     unsigned long long* hist, unsigned long long* pairs, void* stream) {
  if (!scores || !truth || !thr || !hist) return MMDA_EINVAL;
  if (N < 0 || C < 1 || C > CALIB_MAXC || K < 1 || K > CALIB_MAXK) return MMDA_EINVAL;
  if (((uintptr_t)hist & 7) || ((uintptr_t)pairs & 7)) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  const int P = (C + 1) * (C + 1);
  const int kc_max = CALIB_WORDS / P < K ? CALIB_WORDS / P : K;   // 28 at C = 16, all of K = 256 up to C = 4
  // a workgroup's 32-bit counts cannot wrap below 2^31 rows a launch
  const int64_t launch_rows = (int64_t)1 << 30;
  for (int64_t at = 0; at < N; at += launch_rows) {
    const int64_t n = N - at < launch_rows ? N - at : launch_rows;
    const int bx = (int)(ceil_div64(n, CALIB_ROWS) < CALIB_GRID_CAP ? ceil_div64(n, CALIB_ROWS) : CALIB_GRID_CAP);
    // few rows: halve the chunk until the launch has some workgroups to spread over (a batch of 32 rows is one tile)
    int kc = kc_max;
    while (kc > 16 && bx * ceil_div(K, kc) < 32) kc = (kc + 1) / 2;
    const int by = 1 + (pairs ? ceil_div(K, kc) : 0);
    hipLaunchKernelGGL(calib_accumulate_kernel, dim3(bx, by), dim3(256), 0, (hipStream_t)stream, scores + at * C, truth + at * C, n, C,
                       thr, K, kc, hist, pairs);
    MMDA_CHECK_LAUNCH("mmda_calib_accumulate");
  }
  return MMDA_OK;
}

extern "C" int mmda_calib_select(const unsigned long long* hist, const unsigned long long* pairs, int C, int K, const float* thr,
                                 int objective, int per_class, float* out_thr, int32_t* out_k, double* table, void* stream) {
  if (!hist || !thr || !out_thr || !out_k) return MMDA_EINVAL;
  if (C < 1 || C > CALIB_MAXC || K < 1 || K > CALIB_MAXK) return MMDA_EINVAL;
  if (objective < MMDA_CALIB_F1 || objective > MMDA_CALIB_ACC) return MMDA_EINVAL;
  if (per_class && objective != MMDA_CALIB_F1 && objective != MMDA_CALIB_WEIGHTED_F1) return MMDA_EINVAL;
  if (objective == MMDA_CALIB_ACC && !pairs) return MMDA_EINVAL;
  if (((uintptr_t)hist & 7) || ((uintptr_t)pairs & 7) || ((uintptr_t)table & 7)) return MMDA_EINVAL;
  static const int column[4] = {1, 4, 7, 0};                    // f1, micro_f1, weighted_f1, acc among the ten keys
  hipLaunchKernelGGL(calib_select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hist, pairs, C, K, thr, column[objective],
                     per_class ? 1 : 0, out_thr, out_k, table);
  MMDA_CHECK_LAUNCH("mmda_calib_select");
  return MMDA_OK;
}

extern "C" int mmda_eval_accumulate_thr(const float* scores, const float* truth, int N, int C, const float* thr_c, float* labels_out,
                                        double* state, void* stream) {
  if (!scores || !truth || !thr_c || !state || N < 0 || C <= 0 || C > CALIB_MAXC || ((uintptr_t)state & 7)) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  int blocks = (N + 255) / 256; if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(eval_counts_thr_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, scores, truth, N, C, thr_c, labels_out,
                     state);
  MMDA_CHECK_LAUNCH("mmda_eval_accumulate_thr");
  return MMDA_OK;
}
