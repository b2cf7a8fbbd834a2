// Threshold calibration on the device (mmda_amd/calibrate.py: ThresholdSweep, Thresholds).  The model decides
// labels = scores > threshold (reference models.py:249, functions.py:112-115; heads_fwd_kernel's fp32 `s > thr`) and everything the
// reference's evaluation reports moves with that cut-off.  Two entry points (the third, mmda_eval_accumulate_thr, is in eval_counts.hip):
//   mmda_calib_accumulate     every cut-off of a grid at once: per class a histogram of score bins split by truth, and per cut-off the
//                             (|y & p|, |y | p|) pair counts of the rows -- all that get_metrics / get_accuracy are functions of
//   mmda_calib_select         one workgroup: the ten figures at every cut-off and the arg max of one of them, written on the device
// The sweep counts in integers only (32-bit LDS atomics per workgroup, 64-bit global adds of the non-zero bins), so its result does not
// depend on the order of arrival: two runs give the same bits.  Sweep and selection use no floating-point atomic.
#include "internal.h"
#include "eval_terms.h"

namespace {

constexpr int CALIB_MAXK = 256;
constexpr int CALIB_ROWS = 32;                // rows of one workgroup tile
constexpr int CALIB_GRID_CAP = 256;           // workgroups along the rows; beyond it a workgroup strides
// One workgroup counts EITHER the histogram (blockIdx.y == 0: C (K + 1) 2 words, at most 16 * 257 * 2) OR the pair table of one chunk
// of thresholds (blockIdx.y - 1: kc (C + 1)^2 words, kc sized on the host to fit), so one array serves both: 32.1 KB, with the grid 33.1.
constexpr int CALIB_WORDS = EVAL_MAXC * (CALIB_MAXK + 1) * 2;

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

// One workgroup of 256 threads, thread k = cut-off k.  Per class: tp[k] = sum_{j > k} hist[c][j][1], fp[k] likewise from [0], by an
// integer suffix scan in LDS; fn from the class's positive total.  The figures are eval_terms.h's decision figures.
__global__ __launch_bounds__(256) void calib_select_kernel(const unsigned long long* __restrict__ hist,
                                                           const unsigned long long* __restrict__ pairs, int C, int K,
                                                           const float* __restrict__ thr, int col, int per_class,
                                                           float* __restrict__ out_thr, int32_t* __restrict__ out_k,
                                                           double* __restrict__ table) {
  __shared__ unsigned long long scan_s[2][CALIB_MAXK];
  __shared__ unsigned long long tot_s[EVAL_MAXC][2];
  __shared__ double f1_s[EVAL_MAXC][CALIB_MAXK];               // per-class F1 at every cut-off: what per_class selects on
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
  DecisionFigures fig;
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
      double prec, rec;
      fig.add((double)tpi, (double)fpi, (double)fni, (double)sup_all, f1_s[c][k], prec, rec);
    }
    __syncthreads();                                            // scan_s is loaded again
  }
  if (live) {
    double row[10];
    unsigned long long num = 0;
    if (pairs) {
      const unsigned long long* pk = pairs + (int64_t)k * (C + 1) * (C + 1);
      for (int a = 1; a <= C; ++a)
        for (int b = a; b <= C; ++b)                            // |y & p| <= |y | p|: the other entries are zero
          num += pk[a * (C + 1) + b] * (unsigned long long)a * (EVAL_LCM / (unsigned long long)b);
    }
    fig.write(C, pairs != nullptr, num, n_rows, row);
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

}  // namespace

extern "C" int mmda_calib_accumulate(const float* scores, const float* truth, int64_t N, int C, const float* thr, int K,
                                     unsigned long long* hist, unsigned long long* pairs, void* stream) {
  if (!scores || !truth || !thr || !hist) return MMDA_EINVAL;
  if (N < 0 || C < 1 || C > EVAL_MAXC || K < 1 || K > CALIB_MAXK) return MMDA_EINVAL;
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
  if (C < 1 || C > EVAL_MAXC || K < 1 || K > CALIB_MAXK) return MMDA_EINVAL;
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
