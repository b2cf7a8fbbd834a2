// Reliability tables and logit scaling on the device (mmda_amd/reliability.py): are the numbers of a score table
// probabilities, and the per-class monotone rescaling q = sigmoid(a z + b) that makes them so.
//   mmda_reliab_accumulate   one launch: the rows of a batch into the state (include/mmda_hip.h gives its layout)
//   mmda_reliab_finish       one workgroup: the state into the figures and the diagram, on the device
//   mmda_scaling_fit         a clear, a prepare launch, max_iter iteration launches: damped Newton on the mean NLL, state on the device
//   mmda_scaling_apply       one launch: the scaled scores, out of place
// Every kernel but apply maps a workgroup of 256 threads onto 16 rows x 16 class lanes: thread (r, c) = (tid >> 4, tid & 15) walks the
// rows 16 (b + k gridDim) + r of class c, lanes c >= C idle.  A class's 16 row lanes lie 4 to a wave, 16 lanes apart: they are added
// by two butterfly steps, ((r0 + r1) + (r2 + r3)), and the four waves in order.  Integer counts go through LDS atomics and one global
// add per non-zero cell and workgroup.  Float64 sums use no atomic (senti.hip's convention): the workgroups leave partials, the last
// one to arrive -- a ticket that is 0 between launches -- adds them in workgroup order.  No workgroup waits for another.
#include "internal.h"
#include "eval_terms.h"

// every float64 expression below is restated in numpy by the tests: a product and a sum stay two roundings
#pragma clang fp contract(off)

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_ROWS = 16, RL_LANES = 16;                       // rows x class lanes of a workgroup
constexpr int RL_WAVES = RL_THREADS / WAVE;
constexpr int RL_GRID_CAP = MMDA_RELIAB_GRID_CAP;                // beyond 16 * 32 = 512 rows a workgroup strides
constexpr int RL_MAXC = MMDA_RELIAB_MAX_CLASSES, RL_MAXM = MMDA_RELIAB_MAX_BINS;
constexpr double RL_FIX = 1099511627776.0;                       // 2^40
static_assert(RL_ROWS * RL_LANES == RL_THREADS && RL_LANES == RL_MAXC && WAVE == 64, "the (row, class) mapping of a workgroup");

__host__ __device__ inline int rl_grid(int64_t N) {
  const int64_t b = (N + RL_ROWS - 1) / RL_ROWS;
  return (int)(b > RL_GRID_CAP ? RL_GRID_CAP : b);
}

// the sum of v over the 4 row lanes a wave holds of each class: afterwards in every lane, read from lanes 0 .. 15
__device__ __forceinline__ double rl_rows_of_wave(double v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

__device__ __forceinline__ double rl_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------------------------------------------------ the collector
__global__ __launch_bounds__(RL_THREADS) void reliab_accumulate_kernel(const float* __restrict__ prob, const float* __restrict__ target,
                                                                       int64_t N, int C, int M, unsigned long long* __restrict__ st,
                                                                       double* __restrict__ parts) {
  __shared__ unsigned cnt_s[RL_MAXC * RL_MAXM], pos_s[RL_MAXC * RL_MAXM], nan_s[RL_MAXC];
  __shared__ unsigned long long sum_s[RL_MAXC * RL_MAXM];
  __shared__ double red_s[RL_WAVES][RL_LANES][2];
  __shared__ int last_s;
  const int tid = threadIdx.x, r = tid >> 4, c = tid & 15, lane = tid & 63, wave = tid >> 6;
  const int cells = C * M;
  for (int k = tid; k < cells; k += RL_THREADS) { cnt_s[k] = 0u; pos_s[k] = 0u; sum_s[k] = 0ull; }
  if (tid < RL_MAXC) nan_s[tid] = 0u;
  __syncthreads();
  double sq = 0.0, nll = 0.0;
  if (c < C) {
    const float fm = (float)M;
    for (int64_t i = (int64_t)blockIdx.x * RL_ROWS + r; i < N; i += (int64_t)gridDim.x * RL_ROWS) {
      float p = prob[i * C + c];
      const bool y = target[i * C + c] > 0.f;
      if (p != p) { atomicAdd(&nan_s[c], 1u); continue; }
      if (!(p > 0.f)) p = 0.f;                                    // negatives and -0
      if (p > 1.f) p = 1.f;
      int j = (int)__fmul_rn(p, fm);
      j = j > M - 1 ? M - 1 : j;
      const double pd = (double)p;
      atomicAdd(&cnt_s[c * M + j], 1u);
      if (y) atomicAdd(&pos_s[c * M + j], 1u);
      atomicAdd(&sum_s[c * M + j], (unsigned long long)rint(pd * RL_FIX));
      const double d = pd - (y ? 1.0 : 0.0);
      sq += d * d;
      nll += -fmax(y ? log(pd) : log(1.0 - pd), -100.0);          // BCELoss's clamp
    }
  }
  sq = rl_rows_of_wave(sq);
  nll = rl_rows_of_wave(nll);
  if (lane < RL_LANES) { red_s[wave][lane][0] = sq; red_s[wave][lane][1] = nll; }
  __syncthreads();
  for (int k = tid; k < cells; k += RL_THREADS) {
    if (cnt_s[k]) {
      unsigned long long* cell = st + 2 + 3 * C + 3 * k;
      atomicAdd(cell, (unsigned long long)cnt_s[k]);
      if (pos_s[k]) atomicAdd(cell + 1, (unsigned long long)pos_s[k]);
      if (sum_s[k]) atomicAdd(cell + 2, sum_s[k]);
    }
  }
  if (tid < C && nan_s[tid]) atomicAdd(st + 2 + tid, (unsigned long long)nan_s[tid]);
  if (tid < 2 * C) {
    const int cc = tid % C, f = tid / C;
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < RL_WAVES; ++w) v += red_s[w][cc][f];
    parts[((int64_t)blockIdx.x * 2 + f) * RL_MAXC + cc] = v;
  }
  if (!last_to_arrive(st, &last_s)) return;
  if (tid < 2 * C) {
    const int cc = tid % C, f = tid / C;
    double t = 0.0;
    for (int b = 0; b < (int)gridDim.x; ++b) t += rl_load(parts + ((int64_t)b * 2 + f) * RL_MAXC + cc);
    double* sf = reinterpret_cast<double*>(st) + 2 + C + f * C;
    sf[cc] += t;
  }
  if (tid == 0) st[0] = 0ull;
}

// one row of figures from M bins' {cnt, pos, sum_p} (three words a bin) and the two sums; no element: NaN but for n and n_nan
__device__ void reliab_row(const unsigned long long* bins, int M, unsigned long long n_nan, double sum_sq, double sum_nll, double* out) {
  unsigned long long n = 0ull, npos = 0ull, sp = 0ull, gap = 0ull;
  double mce = -1.0;
  for (int j = 0; j < M; ++j) {
    const unsigned long long cnt = bins[3 * j], pos = bins[3 * j + 1], b = bins[3 * j + 2];
    const unsigned long long a = pos << 40;
    const unsigned long long d = a > b ? a - b : b - a;
    n += cnt; npos += pos; sp += b; gap += d;
    if (cnt) {
      const double m = (double)d / (RL_FIX * (double)cnt);
      mce = m > mce ? m : mce;
    }
  }
  const double nan = __builtin_nan(""), dn = (double)n;
  out[0] = dn;
  out[1] = (double)n_nan;
  out[2] = n ? (double)npos / dn : nan;
  out[3] = n ? (double)sp / (RL_FIX * dn) : nan;
  out[4] = n ? (double)gap / (RL_FIX * dn) : nan;
  out[5] = n ? mce : nan;
  out[6] = n ? sum_sq / dn : nan;
  out[7] = n ? sum_nll / dn : nan;
}

__global__ __launch_bounds__(WAVE) void reliab_finish_kernel(const unsigned long long* __restrict__ st, int C, int M,
                                                              double* __restrict__ fig, double* __restrict__ diagram) {
  __shared__ unsigned long long pool_s[RL_MAXM][3];
  const int tid = threadIdx.x;
  constexpr int F = MMDA_RELIAB_FIGURES;
  const unsigned long long* cells = st + 2 + 3 * C;
  const double* sf = reinterpret_cast<const double*>(st) + 2 + C;
  if (tid < C) reliab_row(cells + 3 * tid * M, M, st[2 + tid], sf[tid], sf[C + tid], fig + tid * F);
  if (tid < M) {                                                 // the pooled bins: integer adds over the classes
    unsigned long long a = 0ull, b = 0ull, s = 0ull;
    for (int c = 0; c < C; ++c) { a += cells[3 * (c * M + tid)]; b += cells[3 * (c * M + tid) + 1]; s += cells[3 * (c * M + tid) + 2]; }
    pool_s[tid][0] = a; pool_s[tid][1] = b; pool_s[tid][2] = s;
  }
  for (int k = tid; k < C * M; k += WAVE) {
    const unsigned long long cnt = cells[3 * k], pos = cells[3 * k + 1], sum = cells[3 * k + 2];
    const double nan = __builtin_nan("");
    diagram[3 * k] = (double)cnt;
    diagram[3 * k + 1] = cnt ? (double)pos / (double)cnt : nan;
    diagram[3 * k + 2] = cnt ? (double)sum / (RL_FIX * (double)cnt) : nan;
  }
  __syncthreads();                                               // the class rows (global, this workgroup's own) and the pooled bins
  if (tid == 0) {
    unsigned long long n_nan = 0ull;
    double sq = 0.0, nll = 0.0;
    for (int c = 0; c < C; ++c) { n_nan += st[2 + c]; sq += sf[c]; nll += sf[C + c]; }
    reliab_row(&pool_s[0][0], M, n_nan, sq, nll, fig + (C + 1) * F);
  }
  if (tid < F) {                                                 // column tid of the means: the classes where it is defined, in class order
    double t = 0.0;
    int k = 0;
    for (int c = 0; c < C; ++c) {
      const double v = fig[c * F + tid];
      if (v == v) { t += v; ++k; }
    }
    fig[C * F + tid] = k ? t / (double)k : __builtin_nan("");
  }
}

// ------------------------------------------------------------------------------------------------------------ the fit
// The work buffer, 8-byte words: [0] ticket  [1] groups still running  [2 + g] n  [18 + g] positives (uint64)
//   [SC_STATE + SC_WORDS g + ..] a group's doubles (SC_*) and its {status, iterations} (two int32 in word SC_INTS)
//   [SC_PARTS + (16 b + g) 6 + k] workgroup b's partial of group g: NLL, g_a, g_b, H_aa, H_ab, H_bb   [SC_Z + i C + c] z
constexpr int SC_N = 2, SC_P = 18, SC_STATE = 34, SC_WORDS = 12;
constexpr int SC_TA = 0, SC_TB = 1, SC_AA = 2, SC_AB = 3, SC_NLL = 4, SC_LAM = 5, SC_G = 6, SC_H = 8, SC_INTS = 11;
constexpr int SC_HEADER = 256, SC_NQ = 6;
constexpr int SC_PARTS = SC_HEADER, SC_Z = SC_PARTS + RL_GRID_CAP * RL_MAXC * SC_NQ;
static_assert(SC_STATE + SC_WORDS * RL_MAXC <= SC_HEADER, "the header holds every group's state");
constexpr double SC_GTOL = 1e-12, SC_LAM0 = 1e-2, SC_LAM_MIN_UP = 1e-3, SC_DIAG_FLOOR = 1e-6;
constexpr double SC_RISE = 1.0 / 8796093022208.0;                // 2^-43: the rounding of a mean NLL's sum, below which it has not risen
constexpr float SC_PLO = 1.1920928955078125e-07f, SC_PHI = 0.99999988079071044921875f;   // 2^-23, 1 - 2^-23

__device__ __forceinline__ double scaling_logit(float p) {
  p = p < SC_PLO ? SC_PLO : p;
  p = p > SC_PHI ? SC_PHI : p;
  const double pd = (double)p;
  return log(pd) - log1p(-pd);
}

__device__ __forceinline__ int* sc_ints(unsigned long long* work, int g) {
  return reinterpret_cast<int*>(work + SC_STATE + SC_WORDS * g + SC_INTS);
}

// what the caller reads: every class the values of its group, the last accepted point
__device__ __forceinline__ void scaling_publish(unsigned long long* work, int C, int per_class, double* a, double* b, int* status,
                                                int* iterations) {
  const int c = threadIdx.x;
  if (c >= C) return;
  const int g = per_class ? c : 0;
  const double* s = reinterpret_cast<const double*>(work) + SC_STATE + SC_WORDS * g;
  a[c] = s[SC_AA]; b[c] = s[SC_AB];
  status[c] = sc_ints(work, g)[0]; iterations[c] = sc_ints(work, g)[1];
}

__global__ __launch_bounds__(RL_THREADS) void scaling_prepare_kernel(const float* __restrict__ prob, const float* __restrict__ target,
                                                                     int64_t N, int C, int per_class, unsigned long long* __restrict__ work,
                                                                     double* a, double* b, int* status, int* iterations) {
  __shared__ unsigned n_s[RL_MAXC], p_s[RL_MAXC];
  __shared__ int last_s;
  const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;
  if (tid < RL_MAXC) { n_s[tid] = 0u; p_s[tid] = 0u; }
  __syncthreads();
  double* z = reinterpret_cast<double*>(work) + SC_Z;
  if (c < C) {
    unsigned n = 0u, np = 0u;
    for (int64_t i = (int64_t)blockIdx.x * RL_ROWS + r; i < N; i += (int64_t)gridDim.x * RL_ROWS) {
      const float p = prob[i * C + c];
      if (p != p) { z[i * C + c] = __builtin_nan(""); continue; }
      z[i * C + c] = scaling_logit(p);
      n += 1u;
      np += target[i * C + c] > 0.f ? 1u : 0u;
    }
    const int g = per_class ? c : 0;
    if (n) atomicAdd(&n_s[g], n);
    if (np) atomicAdd(&p_s[g], np);
  }
  __syncthreads();
  if (tid < RL_MAXC) {
    if (n_s[tid]) atomicAdd(work + SC_N + tid, (unsigned long long)n_s[tid]);
    if (p_s[tid]) atomicAdd(work + SC_P + tid, (unsigned long long)p_s[tid]);
  }
  if (!last_to_arrive(work, &last_s)) return;
  const int G = per_class ? C : 1;
  if (tid < G) {
    const unsigned long long n = __hip_atomic_load(work + SC_N + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long np = __hip_atomic_load(work + SC_P + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double* s = reinterpret_cast<double*>(work) + SC_STATE + SC_WORDS * tid;
    s[SC_TA] = 1.0; s[SC_TB] = 0.0; s[SC_AA] = 1.0; s[SC_AB] = 0.0;
    s[SC_NLL] = __builtin_inf(); s[SC_LAM] = SC_LAM0;
    for (int k = SC_G; k < SC_INTS; ++k) s[k] = 0.0;
    sc_ints(work, tid)[0] = np == 0ull || np == n ? MMDA_SCALING_DEGENERATE : MMDA_SCALING_MAXITER;
    sc_ints(work, tid)[1] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long running = 0ull;
    for (int g = 0; g < G; ++g) running += sc_ints(work, g)[0] == MMDA_SCALING_MAXITER ? 1ull : 0ull;
    work[1] = running;
    work[0] = 0ull;
  }
  scaling_publish(work, C, per_class, a, b, status, iterations);
}

// One damped Newton (Levenberg-Marquardt) step of a group from the sums of its trial point; mmda_amd/reliability.py: _lm_update is
// the same in numpy.
__device__ void scaling_update(double* s, int* ints, const double* tot, double n, int platt) {
  const double f = tot[0] / n, ga = tot[1] / n, gb = tot[2] / n, haa = tot[3] / n, hab = tot[4] / n, hbb = tot[5] / n;
  ints[1] += 1;
  if (f <= s[SC_NLL] + fabs(s[SC_NLL]) * SC_RISE) {              // a NaN is a rise
    s[SC_AA] = s[SC_TA]; s[SC_AB] = s[SC_TB]; s[SC_NLL] = f;
    s[SC_G] = ga; s[SC_G + 1] = gb; s[SC_H] = haa; s[SC_H + 1] = hab; s[SC_H + 2] = hbb;
    s[SC_LAM] = s[SC_LAM] * 0.1;
    const double gmax = platt ? fmax(fabs(ga), fabs(gb)) : fabs(ga);
    if (gmax <= SC_GTOL) { ints[0] = MMDA_SCALING_OK; return; }
  } else {
    s[SC_LAM] = fmax(s[SC_LAM] * 10.0, SC_LAM_MIN_UP);
  }
  const double lam = s[SC_LAM];
  const double daa = s[SC_H] + lam * fmax(s[SC_H], SC_DIAG_FLOOR);
  if (!platt) {
    s[SC_TA] = s[SC_AA] - s[SC_G] / daa;
    s[SC_TB] = s[SC_AB];
    return;
  }
  const double dbb = s[SC_H + 2] + lam * fmax(s[SC_H + 2], SC_DIAG_FLOOR), hab0 = s[SC_H + 1];
  const double det = daa * dbb - hab0 * hab0;
  double da, db;
  if (det > 0.0) {
    da = (dbb * s[SC_G] - hab0 * s[SC_G + 1]) / det;
    db = (daa * s[SC_G + 1] - hab0 * s[SC_G]) / det;
  } else {
    da = s[SC_G] / daa;
    db = s[SC_G + 1] / dbb;
  }
  s[SC_TA] = s[SC_AA] - da;
  s[SC_TB] = s[SC_AB] - db;
}

__global__ __launch_bounds__(RL_THREADS) void scaling_iterate_kernel(const float* __restrict__ target, int64_t N, int C, int platt,
                                                                     int per_class, unsigned long long* __restrict__ work, double* a,
                                                                     double* b, int* status, int* iterations) {
  __shared__ double red_s[RL_WAVES][RL_LANES][SC_NQ];
  __shared__ double cls_s[RL_LANES][SC_NQ];
  __shared__ double tot_s[RL_MAXC][SC_NQ];
  __shared__ int last_s;
  if (work[1] == 0ull) return;                                   // every group frozen: written by an earlier launch, the same for all
  const int tid = threadIdx.x, r = tid >> 4, c = tid & 15, lane = tid & 63, wave = tid >> 6;
  const int G = per_class ? C : 1, g = per_class ? c : 0;
  double* wd = reinterpret_cast<double*>(work);
  const double* z = wd + SC_Z;
  double acc[SC_NQ];
#pragma unroll
  for (int k = 0; k < SC_NQ; ++k) acc[k] = 0.0;
  if (c < C && sc_ints(work, g)[0] == MMDA_SCALING_MAXITER) {
    const double pa = wd[SC_STATE + SC_WORDS * g + SC_TA], pb = wd[SC_STATE + SC_WORDS * g + SC_TB];
    for (int64_t i = (int64_t)blockIdx.x * RL_ROWS + r; i < N; i += (int64_t)gridDim.x * RL_ROWS) {
      const double zi = z[i * C + c];
      if (zi != zi) continue;
      const bool y = target[i * C + c] > 0.f;
      const double t = pa * zi + pb;
      const double e = exp(-fabs(t)), d = 1.0 / (1.0 + e);
      const double q = t >= 0.0 ? d : e * d, w = e * d * d;
      const double res = q - (y ? 1.0 : 0.0);
      acc[0] += fmax(y ? -t : t, 0.0) + log1p(e);
      acc[1] += res * zi;
      acc[2] += res;
      acc[3] += w * zi * zi;
      acc[4] += w * zi;
      acc[5] += w;
    }
  }
#pragma unroll
  for (int k = 0; k < SC_NQ; ++k) {
    const double v = rl_rows_of_wave(acc[k]);
    if (lane < RL_LANES) red_s[wave][lane][k] = v;
  }
  __syncthreads();
  if (tid < RL_LANES * SC_NQ) {
    const int cc = tid / SC_NQ, k = tid % SC_NQ;
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < RL_WAVES; ++w) v += red_s[w][cc][k];
    cls_s[cc][k] = v;
  }
  __syncthreads();
  if (tid < G * SC_NQ) {
    const int gg = tid / SC_NQ, k = tid % SC_NQ;
    double v;
    if (per_class) {
      v = cls_s[gg][k];
    } else {
      v = 0.0;
      for (int cc = 0; cc < C; ++cc) v += cls_s[cc][k];
    }
    wd[SC_PARTS + ((int64_t)blockIdx.x * RL_MAXC + gg) * SC_NQ + k] = v;
  }
  if (!last_to_arrive(work, &last_s)) return;
  if (tid < G * SC_NQ) {
    const int gg = tid / SC_NQ, k = tid % SC_NQ;
    double t = 0.0;
    for (int bb = 0; bb < (int)gridDim.x; ++bb) t += rl_load(wd + SC_PARTS + ((int64_t)bb * RL_MAXC + gg) * SC_NQ + k);
    tot_s[gg][k] = t;
  }
  __syncthreads();
  if (tid < G && sc_ints(work, tid)[0] == MMDA_SCALING_MAXITER)
    scaling_update(wd + SC_STATE + SC_WORDS * tid, sc_ints(work, tid), tot_s[tid], (double)work[SC_N + tid], platt);
  __syncthreads();
  if (tid == 0) {
    unsigned long long running = 0ull;
    for (int gg = 0; gg < G; ++gg) running += sc_ints(work, gg)[0] == MMDA_SCALING_MAXITER ? 1ull : 0ull;
    work[1] = running;
    work[0] = 0ull;
  }
  scaling_publish(work, C, per_class, a, b, status, iterations);
}

__global__ __launch_bounds__(RL_THREADS) void scaling_apply_kernel(const float* __restrict__ prob, const double* __restrict__ a,
                                                                   const double* __restrict__ b, int64_t total, int C,
                                                                   float* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * RL_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * RL_THREADS) {
    const float p = prob[e];
    if (p != p) { out[e] = p; continue; }
    const int c = (int)(e % C);
    const double t = a[c] * scaling_logit(p) + b[c];
    const double ex = exp(-fabs(t)), d = 1.0 / (1.0 + ex);
    out[e] = (float)(t >= 0.0 ? d : ex * d);
  }
}

bool rl_shape_ok(int64_t N, int C) { return C >= 1 && C <= RL_MAXC && N >= 0 && N <= MMDA_RELIAB_MAX_ROWS; }
bool rl_aligned(const void* p, uintptr_t a) { return p && !((uintptr_t)p & (a - 1)); }

}  // namespace

extern "C" int mmda_reliab_accumulate(const float* prob, const float* target, int64_t N, int C, int M, void* state, void* stream) {
  if (!rl_aligned(prob, 4) || !rl_aligned(target, 4) || !rl_aligned(state, 8) || !rl_shape_ok(N, C) || M < 1 || M > RL_MAXM)
    return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  double* parts = reinterpret_cast<double*>(mmda_scratch_get((hipStream_t)stream, sizeof(double) * RL_GRID_CAP * 2 * RL_MAXC));
  if (!parts) return MMDA_ELAUNCH;
  hipLaunchKernelGGL(reliab_accumulate_kernel, dim3(rl_grid(N)), dim3(RL_THREADS), 0, (hipStream_t)stream, prob, target, N, C, M,
                     reinterpret_cast<unsigned long long*>(state), parts);
  MMDA_CHECK_LAUNCH("mmda_reliab_accumulate");
  return MMDA_OK;
}

extern "C" int mmda_reliab_finish(const void* state, int C, int M, double* figures, double* diagram, void* stream) {
  if (!rl_aligned(state, 8) || !rl_aligned(figures, 8) || !rl_aligned(diagram, 8) || C < 1 || C > RL_MAXC || M < 1 || M > RL_MAXM)
    return MMDA_EINVAL;
  hipLaunchKernelGGL(reliab_finish_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(state),
                     C, M, figures, diagram);
  MMDA_CHECK_LAUNCH("mmda_reliab_finish");
  return MMDA_OK;
}

extern "C" int64_t mmda_scaling_work_bytes(int64_t N, int C) {
  if (!rl_shape_ok(N, C)) return -1;
  return (int64_t)sizeof(double) * (SC_Z + N * C);
}

extern "C" int mmda_scaling_fit(const float* prob, const float* target, int64_t N, int C, int how, int per_class, int max_iter, void* work,
                                int64_t work_bytes, double* a, double* b, int32_t* status, int32_t* iterations, void* stream) {
  if (!rl_aligned(prob, 4) || !rl_aligned(target, 4) || !rl_aligned(work, 8) || !rl_aligned(a, 8) || !rl_aligned(b, 8) ||
      !rl_aligned(status, 4) || !rl_aligned(iterations, 4) || !rl_shape_ok(N, C))
    return MMDA_EINVAL;
  if ((how != MMDA_SCALING_TEMPERATURE && how != MMDA_SCALING_PLATT) || max_iter < 1 || max_iter > MMDA_SCALING_MAX_ITER ||
      work_bytes < mmda_scaling_work_bytes(N, C))
    return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* w = reinterpret_cast<unsigned long long*>(work);
  if (hipMemsetAsync(work, 0, sizeof(double) * SC_HEADER, s) != hipSuccess) {
    mmda_set_error("mmda_scaling_fit", hipGetLastError());
    return MMDA_ELAUNCH;
  }
  const int grid = rl_grid(N), pc = per_class ? 1 : 0;
  hipLaunchKernelGGL(scaling_prepare_kernel, dim3(grid), dim3(RL_THREADS), 0, s, prob, target, N, C, pc, w, a, b, status, iterations);
  MMDA_CHECK_LAUNCH("mmda_scaling_fit");
  for (int it = 0; it < max_iter; ++it)
    hipLaunchKernelGGL(scaling_iterate_kernel, dim3(grid), dim3(RL_THREADS), 0, s, target, N, C, how == MMDA_SCALING_PLATT ? 1 : 0, pc, w,
                       a, b, status, iterations);
  MMDA_CHECK_LAUNCH("mmda_scaling_fit");
  return MMDA_OK;
}

extern "C" int mmda_scaling_apply(const float* prob, const double* a, const double* b, int64_t N, int C, float* out, void* stream) {
  if (!rl_aligned(prob, 4) || !rl_aligned(a, 8) || !rl_aligned(b, 8) || !rl_aligned(out, 4) || !rl_shape_ok(N, C)) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  hipLaunchKernelGGL(scaling_apply_kernel, dim3(stream_blocks(N * C)), dim3(RL_THREADS), 0, (hipStream_t)stream, prob, a, b, N * C, C, out);
  MMDA_CHECK_LAUNCH("mmda_scaling_apply");
  return MMDA_OK;
}
