// Bootstrap intervals and paired tests on the device (mmda_amd/bootstrap.py): how far a figure of a report would move on
// another draw of the split.  The non-parametric bootstrap over the rows: replicate r draws n rows with replacement,
//   u = rng_u32(seed, SITE_BOOTSTRAP, ((uint64)r << 32) + k),  j(r, k) = ((uint64)u * n) >> 32,  k = 0 .. n - 1
// (the multiply-high map: non-uniform by at most n / 2^32), so a replicate depends on (seed, r, n) alone -- not on R, C, the table or the
// report -- and two reports over the same (seed, n) are a paired comparison.  Replicate R is the identity, j(R, k) = k: the point
// estimate through the same kernels.  Entry points:
//   mmda_boot_pack     (labels, truth) (n, C) -> one 32-bit code per row: bit c = predicted, bit 16 + c = true
//   mmda_boot_counts   per replicate the integer state tp[C], fp[C], fn[C], acc_num, n of the drawn rows
//   mmda_boot_figures  the states -> (R + 1, 10 + 3 C) float64: get_metrics' ten figures, then f1 / precision / recall per class
//   mmda_boot_rank     per (replicate, class) the ranking figures of ranking.py under the replicate's row weights
//   mmda_boot_summary  an (R + 1, F) figure table (or the difference of two) -> point, mean, std, percentile interval, defined count
//   mmda_boot_plan_describe  the form mmda_boot_counts gives a shape (host only; the launcher reads the same function)
// Everything counted is an integer, combined by integer adds only, so no state depends on the form or on the order of arrival.  The
// floating-point sums (the two AP sums, the mean and std of a summary) are added in an order that is a function of the shape alone.
#include "internal.h"
#include "dynamic_lds.h"
#include "eval_terms.h"

// No product is fused into a sum in this file: the host restatements (numpy) round every product and every sum on its own.  Plain
// operators under this pragma, not __dmul_rn / __dadd_rn: those inline to operators that carry the headers' contraction mode.
#pragma clang fp contract(off)

namespace {

enum { SITE_BOOTSTRAP = 12 };                  // the next id after modality.hip's SITE_MODALITY

constexpr int64_t BOOT_MAXN = (int64_t)1 << 20;
constexpr int BOOT_MAXR = 8192;                // replicates: what one workgroup of mmda_boot_summary sorts in 64 KiB of LDS
constexpr int BOOT_LDS_ROWS = 16384;           // the code table sits in LDS up to here (64 KiB); the ranking kernel's row limit
constexpr int BOOT_THREADS = 256;              // of a workgroup of the count kernel
constexpr int BOOT_DRAWS_PER_WG = 4096;        // a replicate is split into workgroups of about this many draws ...
constexpr int BOOT_MAX_WGS = 16;               // ... at most this many
constexpr int BOOT_RANK_THREADS = 1024;
constexpr int BOOT_SUM_THREADS = 1024;

enum { BOOT_FORM_AUTO = 0, BOOT_FORM_LDS = 1, BOOT_FORM_GLOBAL = 2 };

__device__ __forceinline__ uint32_t boot_draw(uint64_t seed, uint32_t r, uint32_t k, uint32_t n) {
  const uint32_t u = rng_u32(seed, SITE_BOOTSTRAP, ((uint64_t)r << 32) + (uint64_t)k);
  return (uint32_t)(((uint64_t)u * (uint64_t)n) >> 32);      // < n
}

// ------------------------------------------------------------------------------------------------ decision figures
__global__ __launch_bounds__(256) void boot_pack_kernel(const float* __restrict__ labels, const float* __restrict__ truth, int64_t n, int C,
                                                        uint32_t* __restrict__ codes) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    uint32_t code = 0u;
    for (int c = 0; c < C; ++c) {
      code |= (labels[i * C + c] > 0.f ? 1u : 0u) << c;
      code |= (truth[i * C + c] > 0.f ? 1u : 0u) << (16 + c);
    }
    codes[i] = code;
  }
}

// grid (wgs, R + 1): workgroup blockIdx.x of replicate blockIdx.y counts the draws k of its share.  LDS: the whole code table is staged
// in dynamic LDS first (n <= BOOT_LDS_ROWS), else every draw gathers its code from memory.  Per thread 48 counters and the Jaccard
// numerator; a wave's sums by shuffles, the workgroup's in 64-bit LDS integers, and from there one 64-bit integer add per non-zero
// word into the replicate's state (cleared by the launcher).
template <bool LDS>
__global__ __launch_bounds__(BOOT_THREADS) void boot_counts_kernel(const uint32_t* __restrict__ codes, int n, int C, int R, uint64_t seed,
                                                                   unsigned long long* __restrict__ state) {
  extern __shared__ uint32_t tab_s[];
  __shared__ unsigned long long acc_s[3 * EVAL_MAXC + 2];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int r = blockIdx.y;
  const int words = 3 * C + 2;
  if (LDS)
    for (int k = tid; k < n; k += BOOT_THREADS) tab_s[k] = codes[k];
  for (int w = tid; w < words; w += BOOT_THREADS) acc_s[w] = 0ull;
  __syncthreads();
  const int per = (n + (int)gridDim.x - 1) / (int)gridDim.x;
  const int k0 = (int)blockIdx.x * per;
  const int k1 = k0 + per < n ? k0 + per : n;
  unsigned tp[EVAL_MAXC], fp[EVAL_MAXC], fn[EVAL_MAXC];
#pragma unroll
  for (int c = 0; c < EVAL_MAXC; ++c) { tp[c] = 0u; fp[c] = 0u; fn[c] = 0u; }
  unsigned long long acc = 0ull;
  unsigned cnt = 0u;
  for (int k = k0 + tid; k < k1; k += BOOT_THREADS) {
    const uint32_t j = r == R ? (uint32_t)k : boot_draw(seed, (uint32_t)r, (uint32_t)k, (uint32_t)n);      // j < n
    const uint32_t code = LDS ? tab_s[j] : codes[j];
    const uint32_t p = code & 0xffffu, y = code >> 16;
    const uint32_t a = p & y, b = p & ~y, d = y & ~p;
#pragma unroll
    for (int c = 0; c < EVAL_MAXC; ++c) { tp[c] += (a >> c) & 1u; fp[c] += (b >> c) & 1u; fn[c] += (d >> c) & 1u; }
    const unsigned uni = (unsigned)__popc(p | y);
    acc += (unsigned long long)(((unsigned)EVAL_LCM / (uni ? uni : 1u)) * (unsigned)__popc(a));
    cnt += 1u;
  }
  auto wsum = [](unsigned v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v += __shfl_xor(v, o);
    return v;
  };
#pragma unroll
  for (int c = 0; c < EVAL_MAXC; ++c) {
    if (c < C) {                                                // uniform
      const unsigned a = wsum(tp[c]), b = wsum(fp[c]), d = wsum(fn[c]);
      if (lane == 0) {
        if (a) atomicAdd(&acc_s[c], (unsigned long long)a);
        if (b) atomicAdd(&acc_s[C + c], (unsigned long long)b);
        if (d) atomicAdd(&acc_s[2 * C + c], (unsigned long long)d);
      }
    }
  }
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) acc += __shfl_xor(acc, o);
  cnt = wsum(cnt);
  if (lane == 0 && cnt) { atomicAdd(&acc_s[3 * C], acc); atomicAdd(&acc_s[3 * C + 1], (unsigned long long)cnt); }
  __syncthreads();
  for (int w = tid; w < words; w += BOOT_THREADS) {
    const unsigned long long v = acc_s[w];
    if (v) atomicAdd(&state[(int64_t)r * words + w], v);
  }
}

// One thread per replicate: eval_terms.h's decision figures of the replicate's state, then the per-class triples.
__global__ __launch_bounds__(64) void boot_figures_kernel(const long long* __restrict__ state, int C, int rows, double* __restrict__ out) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= rows) return;
  const long long* st = state + (int64_t)r * (3 * C + 2);
  double* o = out + (int64_t)r * (10 + 3 * C);
  double sup_sum = 0.0;
  for (int c = 0; c < C; ++c) sup_sum += (double)(st[c] + st[2 * C + c]);
  DecisionFigures fig;
  for (int c = 0; c < C; ++c)
    fig.add((double)st[c], (double)st[C + c], (double)st[2 * C + c], sup_sum, o[10 + c], o[10 + C + c], o[10 + 2 * C + c]);
  const long long n = st[3 * C + 1];
  fig.write(C, n > 0, (unsigned long long)st[3 * C], (unsigned long long)n, o);
}

// ------------------------------------------------------------------------------------------------ ranking figures
// One workgroup per (replicate blockIdx.x, class blockIdx.y).  The class's rows are known in SORTED order (descending score, ties
// adjacent): inv[row] = sorted position, and per sorted position first / last of its tie group and pos = the row is a positive.
//   1. the replicate's draws are histogrammed into W[position] (dynamic LDS, 32-bit integer adds);
//   2. W and W * (1 - pos) are scanned over the positions, tile by tile of one position per thread, in place: afterwards
//      W[p] = weight of the positions <= p, SN[p] = weight of the negatives among them;
//   3. a row at p with weight w = W[p] - W[p - 1] > 0 and tie group [a, b] has GN = SN[a - 1], GN + EN = SN[b],
//      GP = W[a - 1] - GN, GP + EP = W[b] - SN[b]: ranking.py's counts of the materialised resample.
// Integer sums and the integer minimum by xor butterfly and wave order; the two fp64 sums thread-strided over the positions, then the
// same tree: their order is a function of n alone.
__global__ __launch_bounds__(BOOT_RANK_THREADS) void boot_rank_kernel(const int32_t* __restrict__ inv, const int32_t* __restrict__ first,
                                                                      const int32_t* __restrict__ last, const int32_t* __restrict__ pos,
                                                                      int n, int C, int R, uint64_t seed, double level,
                                                                      double* __restrict__ out) {
  constexpr int T = BOOT_RANK_THREADS, WAVES = T / WAVE;
  extern __shared__ uint32_t rank_s[];
  uint32_t* W = rank_s;
  uint32_t* SN = rank_s + n;
  __shared__ uint32_t wt_s[WAVES], wn_s[WAVES];
  __shared__ unsigned long long num_s[WAVES], min_s[WAVES];
  __shared__ double ap_s[WAVES], apn_s[WAVES];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int r = blockIdx.x, c = blockIdx.y;
  const int32_t* inv_c = inv + (int64_t)c * n;
  const int32_t* first_c = first + (int64_t)c * n;
  const int32_t* last_c = last + (int64_t)c * n;
  const int32_t* pos_c = pos + (int64_t)c * n;
  for (int p = tid; p < n; p += T) W[p] = 0u;
  __syncthreads();
  for (int k = tid; k < n; k += T) {
    const uint32_t j = r == R ? (uint32_t)k : boot_draw(seed, (uint32_t)r, (uint32_t)k, (uint32_t)n);      // j < n
    const uint32_t q = (uint32_t)inv_c[j];
    if (q < (uint32_t)n) atomicAdd(&W[q], 1u);
  }
  __syncthreads();
  uint32_t carry_w = 0u, carry_n = 0u;
  for (int base = 0; base < n; base += T) {
    const int p = base + tid;
    uint32_t sw = p < n ? W[p] : 0u;
    uint32_t sn = (p < n && pos_c[p] == 0) ? sw : 0u;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      const uint32_t a = __shfl_up(sw, o), b = __shfl_up(sn, o);
      if (lane >= o) { sw += a; sn += b; }
    }
    if (lane == WAVE - 1) { wt_s[wave] = sw; wn_s[wave] = sn; }
    __syncthreads();
    uint32_t off_w = carry_w, off_n = carry_n;
    for (int i = 0; i < WAVES; ++i) {
      if (i < wave) { off_w += wt_s[i]; off_n += wn_s[i]; }
      carry_w += wt_s[i]; carry_n += wn_s[i];
    }
    if (p < n) { W[p] = off_w + sw; SN[p] = off_n + sn; }
    __syncthreads();                                            // the wave totals are read; W / SN of the tile are written
  }
  const unsigned long long Nn = carry_n, P = (unsigned long long)carry_w - carry_n;
  RankFigures<WAVES> fig(level, P);
  for (int p = tid; p < n; p += T) {
    const unsigned long long w = W[p] - (p ? W[p - 1] : 0u);
    if (!w) continue;
    int a = first_c[p], b = last_c[p];
    a = a < 0 ? 0 : a > p ? p : a;                              // a <= p <= b < n whatever the tables hold
    b = b < p ? p : b >= n ? n - 1 : b;
    const unsigned long long wb = W[b], gnen = SN[b];
    const unsigned long long wa = a ? W[a - 1] : 0u, gn = a ? SN[a - 1] : 0u;
    if (pos_c[p] != 0) fig.positive(w, wb - gnen, gn, gnen, Nn);
    else fig.negative(w, wa - gn, gn, P, Nn);
  }
  if (fig.reduce(num_s, min_s, ap_s, apn_s)) fig.write(P, Nn, out + ((int64_t)r * (C + 1) + c) * 6);
}

// Row C of every replicate's table, one thread per replicate.
__global__ __launch_bounds__(64) void boot_rank_macro_kernel(int C, int rows, double* __restrict__ out) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r < rows) rank_macro_row(C, out + (int64_t)r * (C + 1) * 6);
}

// ------------------------------------------------------------------------------------------------ summaries
// One workgroup per figure f.  x_r = A[r][f] (B: A[r][f] - B[r][f], NaN where either is), r < R; the defined ones are sorted in LDS as
// monotone 64-bit keys (a NaN and the padding up to a power of two take the highest key), then ONE thread adds them in sorted order:
// mean, the two-pass std (ddof 1), and the two percentiles by linear interpolation at h = (m - 1) q.  ncols 6: point, mean, std, lo, hi,
// defined; ncols 9: and p_le, p_ge, p_two from the integer counts of x <= 0 and x >= 0.
__device__ __forceinline__ unsigned long long boot_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double boot_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}
__device__ __forceinline__ double boot_percentile(const unsigned long long* key, int m, double q) {
  const double h = (double)(m - 1) * q;
  int a = (int)floor(h);
  a = a < 0 ? 0 : a > m - 1 ? m - 1 : a;
  const int b = a + 1 < m ? a + 1 : m - 1;
  const double xa = boot_unkey(key[a]), xb = boot_unkey(key[b]);
  return xa + (h - (double)a) * (xb - xa);
}

__global__ __launch_bounds__(BOOT_SUM_THREADS) void boot_summary_kernel(const double* __restrict__ A, const double* __restrict__ B, int R,
                                                                        int F, int Rp, double q_lo, double q_hi, int ncols,
                                                                        double* __restrict__ out) {
  extern __shared__ unsigned long long key_s[];
  __shared__ int cnt_s[3];
  const int tid = threadIdx.x, f = blockIdx.x;
  if (tid < 3) cnt_s[tid] = 0;
  __syncthreads();
  int m_t = 0, le_t = 0, ge_t = 0;
  for (int i = tid; i < Rp; i += BOOT_SUM_THREADS) {
    unsigned long long k = ~0ull;
    if (i < R) {
      double v = A[(int64_t)i * F + f];
      if (B) v = v - B[(int64_t)i * F + f];
      if (v == v) { k = boot_key(v); ++m_t; le_t += v <= 0.0 ? 1 : 0; ge_t += v >= 0.0 ? 1 : 0; }
    }
    key_s[i] = k;
  }
  if (m_t) atomicAdd(&cnt_s[0], m_t);
  if (le_t) atomicAdd(&cnt_s[1], le_t);
  if (ge_t) atomicAdd(&cnt_s[2], ge_t);
  __syncthreads();
  for (int k = 2; k <= Rp; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < Rp; i += BOOT_SUM_THREADS) {
        const int x = i ^ j;
        if (x > i) {
          const unsigned long long a = key_s[i], b = key_s[x];
          const bool up = (i & k) == 0;
          if (up ? a > b : a < b) { key_s[i] = b; key_s[x] = a; }
        }
      }
      __syncthreads();
    }
  }
  if (tid != 0) return;
  const int m = cnt_s[0];
  const double nan = __builtin_nan("");
  double* row = out + (int64_t)f * ncols;
  double point = A[(int64_t)R * F + f];
  if (B) point = point - B[(int64_t)R * F + f];
  double mean = nan, sd = nan, lo = nan, hi = nan;
  if (m > 0) {
    double s = 0.0;
    for (int i = 0; i < m; ++i) s = s + boot_unkey(key_s[i]);
    mean = s / (double)m;
    if (m > 1) {
      double ss = 0.0;
      for (int i = 0; i < m; ++i) {
        const double d = boot_unkey(key_s[i]) - mean;
        ss = ss + d * d;
      }
      sd = sqrt(ss / (double)(m - 1));
    }
    lo = boot_percentile(key_s, m, q_lo);
    hi = boot_percentile(key_s, m, q_hi);
  }
  row[0] = point; row[1] = mean; row[2] = sd; row[3] = lo; row[4] = hi; row[5] = (double)m;
  if (ncols == 9) {
    const double p_le = (double)(1 + cnt_s[1]) / (double)(m + 1), p_ge = (double)(1 + cnt_s[2]) / (double)(m + 1);
    const double two = 2.0 * (p_le < p_ge ? p_le : p_ge);
    row[6] = p_le; row[7] = p_ge; row[8] = two < 1.0 ? two : 1.0;
  }
}

bool boot_shape_ok(int64_t n, int C, int R) { return n >= 1 && n <= BOOT_MAXN && C >= 1 && C <= EVAL_MAXC && R >= 1 && R <= BOOT_MAXR; }

}  // namespace

extern "C" int mmda_boot_plan_describe(int64_t n, int C, int R, mmda_boot_plan* out) {
  if (!out || !boot_shape_ok(n, C, R)) return MMDA_EINVAL;
  mmda_boot_plan p{};
  p.form = n <= BOOT_LDS_ROWS ? BOOT_FORM_LDS : BOOT_FORM_GLOBAL;
  p.threads = BOOT_THREADS;
  int wgs = (int)ceil_div64(n, BOOT_DRAWS_PER_WG);
  p.wgs_per_replicate = wgs > BOOT_MAX_WGS ? BOOT_MAX_WGS : wgs;
  p.lds_bytes = p.form == BOOT_FORM_LDS ? (int)n * (int)sizeof(uint32_t) : 0;
  p.state_words = 3 * C + 2;
  p.lds_rows = BOOT_LDS_ROWS;
  p.rank_lds_bytes = n <= BOOT_LDS_ROWS ? 2 * (int)n * (int)sizeof(uint32_t) : 0;
  p.max_replicates = BOOT_MAXR;
  *out = p;
  return MMDA_OK;
}

extern "C" int mmda_boot_pack(const float* labels, const float* truth, int64_t n, int C, uint32_t* codes, void* stream) {
  if (!labels || !truth || !codes || !boot_shape_ok(n, C, 1)) return MMDA_EINVAL;
  hipLaunchKernelGGL(boot_pack_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, labels, truth, n, C, codes);
  MMDA_CHECK_LAUNCH("mmda_boot_pack");
  return MMDA_OK;
}

extern "C" int mmda_boot_counts(const uint32_t* codes, int64_t n, int C, int R, uint64_t seed, int form, int64_t* state, void* stream) {
  if (!codes || !state || ((uintptr_t)state & 7)) return MMDA_EINVAL;
  mmda_boot_plan p;
  if (mmda_boot_plan_describe(n, C, R, &p) != MMDA_OK) return MMDA_EINVAL;
  if (form != BOOT_FORM_AUTO && form != BOOT_FORM_LDS && form != BOOT_FORM_GLOBAL) return MMDA_EINVAL;
  if (form == BOOT_FORM_LDS && n > BOOT_LDS_ROWS) return MMDA_EINVAL;
  if (form == BOOT_FORM_AUTO) form = p.form;
  const hipError_t e = hipMemsetAsync(state, 0, sizeof(int64_t) * (size_t)(R + 1) * (size_t)p.state_words, (hipStream_t)stream);
  if (e != hipSuccess) { mmda_set_error("mmda_boot_counts", e); return MMDA_ELAUNCH; }
  const dim3 grid(p.wgs_per_replicate, R + 1);
  unsigned long long* st = reinterpret_cast<unsigned long long*>(state);
  if (form == BOOT_FORM_LDS) {
    const size_t lds = (size_t)n * sizeof(uint32_t);
    ensure_dynamic_lds(boot_counts_kernel<true>, lds);
    hipLaunchKernelGGL(boot_counts_kernel<true>, grid, dim3(BOOT_THREADS), lds, (hipStream_t)stream, codes, (int)n, C, R, seed, st);
  } else {
    hipLaunchKernelGGL(boot_counts_kernel<false>, grid, dim3(BOOT_THREADS), 0, (hipStream_t)stream, codes, (int)n, C, R, seed, st);
  }
  MMDA_CHECK_LAUNCH("mmda_boot_counts");
  return MMDA_OK;
}

extern "C" int mmda_boot_figures(const int64_t* state, int C, int R, double* out, void* stream) {
  if (!state || !out || !boot_shape_ok(1, C, R) || ((uintptr_t)state & 7) || ((uintptr_t)out & 7)) return MMDA_EINVAL;
  hipLaunchKernelGGL(boot_figures_kernel, dim3(ceil_div(R + 1, 64)), dim3(64), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(state), C, R + 1, out);
  MMDA_CHECK_LAUNCH("mmda_boot_figures");
  return MMDA_OK;
}

extern "C" int mmda_boot_rank(const int32_t* inv, const int32_t* first, const int32_t* last, const int32_t* pos, int64_t n, int C, int R,
                              uint64_t seed, double tpr_level, double* out, void* stream) {
  if (!inv || !first || !last || !pos || !out || ((uintptr_t)out & 7)) return MMDA_EINVAL;
  if (!boot_shape_ok(n, C, R) || n > BOOT_LDS_ROWS || !(tpr_level > 0.0 && tpr_level <= 1.0)) return MMDA_EINVAL;
  const size_t lds = 2 * (size_t)n * sizeof(uint32_t);
  ensure_dynamic_lds(boot_rank_kernel, lds);
  hipLaunchKernelGGL(boot_rank_kernel, dim3(R + 1, C), dim3(BOOT_RANK_THREADS), lds, (hipStream_t)stream, inv, first, last, pos, (int)n, C, R,
                     seed, tpr_level, out);
  MMDA_CHECK_LAUNCH("mmda_boot_rank");
  hipLaunchKernelGGL(boot_rank_macro_kernel, dim3(ceil_div(R + 1, 64)), dim3(64), 0, (hipStream_t)stream, C, R + 1, out);
  MMDA_CHECK_LAUNCH("mmda_boot_rank");
  return MMDA_OK;
}

extern "C" int mmda_boot_summary(const double* a, const double* b, int R, int F, double q_lo, double q_hi, int ncols, double* out,
                                 void* stream) {
  if (!a || !out || ((uintptr_t)a & 7) || ((uintptr_t)b & 7) || ((uintptr_t)out & 7)) return MMDA_EINVAL;
  if (R < 1 || R > BOOT_MAXR || F < 1 || (ncols != 6 && ncols != 9)) return MMDA_EINVAL;
  if (!(q_lo >= 0.0 && q_lo <= 1.0 && q_hi >= 0.0 && q_hi <= 1.0)) return MMDA_EINVAL;
  int Rp = 2;
  while (Rp < R) Rp <<= 1;
  const size_t lds = (size_t)Rp * sizeof(unsigned long long);
  ensure_dynamic_lds(boot_summary_kernel, lds);
  hipLaunchKernelGGL(boot_summary_kernel, dim3(F), dim3(BOOT_SUM_THREADS), lds, (hipStream_t)stream, a, b, R, F, Rp, q_lo, q_hi, ncols, out);
  MMDA_CHECK_LAUNCH("mmda_boot_summary");
  return MMDA_OK;
}
