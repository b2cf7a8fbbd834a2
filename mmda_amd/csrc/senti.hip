// The sentiment table on the device (mmda_amd/sentiment.py: SentimentEval): the nine figures of the reference's
// eval_mosei_senti (src/utils/eval_metrics.py) from one state that a launch per batch adds to.
//   mmda_senti_accumulate   one launch: the rows of a batch into the state
//   mmda_senti_finish       one workgroup: the state into the figures, on the device
// The state is MMDA_SENTI_STATE_WORDS 8-byte words, cleared by the caller:
//   [0] n  [1] n_nonzero (truth != 0)  [2] Acc-7 hits  [3] Acc-5 hits  [4..7] the 2x2 table of (truth >= 0, pred >= 0) over all rows
//   [8..11] the table of (truth > 0, pred > 0) over the rows with truth != 0  [12] n_extreme (|truth| > 2)  [13] ticket (0 between launches)
//   -- unsigned 64-bit, table index 2 * truth bit + pred bit --
//   [16] sum |p - t|  [17] the same over the extreme rows  [18] sum p  [19] sum t  [20] sum p^2  [21] sum t^2  [22] sum p t   -- doubles
// Counts are integer adds: they do not depend on the order of arrival or on how the rows are split into batches.  The float64 sums
// use no atomic (loss_parts_add's convention, losses.hip): a thread adds its rows in row order, a workgroup its threads in a fixed
// order, the workgroups leave partials, and the last one to arrive adds them in workgroup order -- the same batches give the same bits.
#include "internal.h"
#include "eval_terms.h"

namespace {

constexpr int SENTI_THREADS = 256;
constexpr int SENTI_GRID_CAP = 32;            // workgroups of a launch; beyond 8192 rows a workgroup strides
constexpr int SENTI_NI = 13, SENTI_NF = 7;    // integer counts, float64 sums
constexpr int SENTI_TICKET = 13, SENTI_F0 = 16;

__global__ __launch_bounds__(SENTI_THREADS) void senti_accumulate_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                                         int64_t N, unsigned long long* __restrict__ st,
                                                                         double* __restrict__ parts) {
  __shared__ unsigned cnt_s[SENTI_NI];
  __shared__ double red_s[SENTI_THREADS / WAVE][SENTI_NF];
  __shared__ int last_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < SENTI_NI) cnt_s[tid] = 0u;
  __syncthreads();
  unsigned c[SENTI_NI];
  double f[SENTI_NF];
#pragma unroll
  for (int k = 0; k < SENTI_NI; ++k) c[k] = 0u;
#pragma unroll
  for (int k = 0; k < SENTI_NF; ++k) f[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * SENTI_THREADS + tid; i < N; i += (int64_t)gridDim.x * SENTI_THREADS) {
    const float pf = pred[i], tf = truth[i];
    const double p = (double)pf, t = (double)tf;
    const double ad = fabs(p - t);
    const bool non0 = tf != 0.f, ext = fabsf(tf) > 2.f;
    c[0] += 1u;
    c[1] += non0 ? 1u : 0u;
    // np.round is half-to-even, as rintf in the default rounding mode; a float's clip and rounding are those of its float64 value
    c[2] += rintf(fminf(fmaxf(pf, -3.f), 3.f)) == rintf(fminf(fmaxf(tf, -3.f), 3.f)) ? 1u : 0u;
    c[3] += rintf(fminf(fmaxf(pf, -2.f), 2.f)) == rintf(fminf(fmaxf(tf, -2.f), 2.f)) ? 1u : 0u;
    c[4 + 2 * (tf >= 0.f ? 1 : 0) + (pf >= 0.f ? 1 : 0)] += 1u;
    if (non0) c[8 + 2 * (tf > 0.f ? 1 : 0) + (pf > 0.f ? 1 : 0)] += 1u;
    c[12] += ext ? 1u : 0u;
    f[0] += ad;
    f[1] += ext ? ad : 0.0;
    f[2] += p; f[3] += t; f[4] += p * p; f[5] += t * t; f[6] += p * t;
  }
#pragma unroll
  for (int k = 0; k < SENTI_NI; ++k)
    if (c[k]) atomicAdd(&cnt_s[k], c[k]);
#pragma unroll
  for (int k = 0; k < SENTI_NF; ++k) {
    const double v = wave_sum_f64(f[k]);
    if (lane == 0) red_s[wave][k] = v;
  }
  __syncthreads();
  if (tid < SENTI_NI && cnt_s[tid]) atomicAdd(&st[tid], (unsigned long long)cnt_s[tid]);
  if (tid < SENTI_NF) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < SENTI_THREADS / WAVE; ++w) v += red_s[w][tid];
    parts[blockIdx.x * SENTI_NF + tid] = v;
  }
  if (!last_to_arrive(&st[SENTI_TICKET], &last_s)) return;
  if (tid < SENTI_NF) {
    double t = 0.0;
    for (int b = 0; b < (int)gridDim.x; ++b) t += __hip_atomic_load(parts + b * SENTI_NF + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double* sf = reinterpret_cast<double*>(st) + SENTI_F0;
    sf[tid] += t;
  }
  if (tid == 0) st[SENTI_TICKET] = 0ull;
}

// sklearn's f1_score(average='weighted') of a binary problem from its 2x2 table T[2 truth + pred]: per label 2 tp / (true + pred), 0 where
// that denominator is 0, weighted by the label's count among the truths.  No row at all: NaN.
__device__ __forceinline__ double senti_weighted_f1(const unsigned long long* T) {
#pragma clang fp contract(off)
  const double tn = (double)T[0], fp = (double)T[1], fn = (double)T[2], tp = (double)T[3];
  const double true0 = tn + fp, true1 = fn + tp, den0 = true0 + (tn + fn), den1 = true1 + (fp + tp);
  const double f0 = den0 > 0.0 ? 2.0 * tn / den0 : 0.0, f1 = den1 > 0.0 ? 2.0 * tp / den1 : 0.0;
  return (f0 * true0 + f1 * true1) / (true0 + true1);
}

// out: mae, corr, acc7, acc5, acc2, f1, acc2_non0, f1_non0, mae_intensity (MMDA_SENTI_FIGURES doubles)
__global__ void senti_finish_kernel(const unsigned long long* __restrict__ st, double* __restrict__ out) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double* sf = reinterpret_cast<const double*>(st) + SENTI_F0;
  const double n = (double)st[0], n0 = (double)st[1], next = (double)st[12];
  const double sp = sf[2], stt = sf[3], spp = sf[4], st2 = sf[5], spt = sf[6];
  out[0] = sf[0] / n;
  // Pearson's r from the raw moments; np.corrcoef clips to [-1, 1] and leaves NaN (a constant column, a single row) a NaN
  const double num = n * spt - sp * stt, vp = n * spp - sp * sp, vt = n * st2 - stt * stt;
  double r = num / (sqrt(vp) * sqrt(vt));
  if (r > 1.0) r = 1.0;
  if (r < -1.0) r = -1.0;
  out[1] = r;
  out[2] = (double)st[2] / n;
  out[3] = (double)st[3] / n;
  out[4] = ((double)st[4] + (double)st[7]) / n;
  out[5] = senti_weighted_f1(st + 4);
  // no row with truth != 0: the reference itself fails there (an empty index array); both figures are NaN by definition
  out[6] = ((double)st[8] + (double)st[11]) / n0;
  out[7] = senti_weighted_f1(st + 8);
  out[8] = sf[1] / next;                                 // no extreme row: 0 / 0, numpy's mean of an empty array
}

}  // namespace

extern "C" int mmda_senti_accumulate(const float* pred, const float* truth, int64_t N, void* state, void* stream) {
  if (!pred || !truth || !state || N < 0 || ((uintptr_t)state & 7) || N > ((int64_t)1 << 40)) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  const int64_t b = ceil_div64(N, SENTI_THREADS);
  const int blocks = (int)(b > SENTI_GRID_CAP ? SENTI_GRID_CAP : b);
  double* parts = reinterpret_cast<double*>(mmda_scratch_get((hipStream_t)stream, sizeof(double) * SENTI_GRID_CAP * SENTI_NF));
  if (!parts) return MMDA_ELAUNCH;
  hipLaunchKernelGGL(senti_accumulate_kernel, dim3(blocks), dim3(SENTI_THREADS), 0, (hipStream_t)stream, pred, truth, N,
                     reinterpret_cast<unsigned long long*>(state), parts);
  MMDA_CHECK_LAUNCH("mmda_senti_accumulate");
  return MMDA_OK;
}

extern "C" int mmda_senti_finish(const void* state, double* out, void* stream) {
  if (!state || !out || ((uintptr_t)state & 7) || ((uintptr_t)out & 7)) return MMDA_EINVAL;
  hipLaunchKernelGGL(senti_finish_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(state), out);
  MMDA_CHECK_LAUNCH("mmda_senti_finish");
  return MMDA_OK;
}
