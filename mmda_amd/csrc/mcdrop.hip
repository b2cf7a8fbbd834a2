// MC-dropout statistics (mmda_amd/uncertainty.py: mc_statistics, MCDropoutPass): K stochastic draws per sample sit in adjacent rows of
// one (B K, W) table -- the fusion block run once at B K columns over rows gathered K times each, so the K copies of a sample see K
// independent masks (the batch column is part of every mask index) -- and ONE launch reduces them to per-SAMPLE float64 tables: mean,
// population variance, the Bernoulli entropy of the mean, the mean entropy of the draws, their difference (the mutual information), the
// share of draws above a threshold, and the draws themselves.  A collector in the style of infer.hip: one row per sample, row dst[b] or
// base + b, 64-bit offsets, nothing checks the rows.  DESIGN.md 4p.
#include "misa_handle.h"

namespace {

constexpr int MC_MAX_K = 256, MC_MAX_W = 64;
constexpr int MC_PER_LANE = MC_MAX_K / 64;       // draws one lane holds: k = lane + 64 j, j = 0 .. 3

struct McArgs {
  const float* p; const float* thr; mmda_mc_out o;
  const int32_t* dst; int64_t base; int B, K, W, bernoulli;
};

// h(q) = -q ln q - (1 - q) ln(1 - q) in nats; h(0) = h(1) = 0 by the limit, a NaN stays a NaN
__device__ __forceinline__ double bernoulli_entropy(double q) {
  if (q == 0.0 || q == 1.0) return 0.0;
  return -q * log(q) - (1.0 - q) * log(1.0 - q);
}

// One wave per (sample b, column w): blockIdx.x = b, the four waves of a workgroup take w = wave, wave + 4, ...  Lane l holds draws
// k = l, l + 64, l + 128, l + 192 (those below K) of its column, widened once to float64, in registers; a lane's partial sum adds them in
// that order and wave_sum_widest_first (common.h: six xor steps, 32 .. 1) adds the 64 partials, so the order of every addition is a
// function of K alone -- not of B, dst or the workgroup -- and two runs give the same bits.  The variance is a second pass over the
// same registers against the finished mean (exactly 0 at K = 1: the mean of one draw is the draw).  A NaN draw reaches every sum of
// its own (b, w) and nothing else; the vote is a count of `p > thr`, which a NaN fails.  No atomics, no LDS, no scratch.
__global__ __launch_bounds__(256) void mc_reduce_kernel(const McArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = (int)blockIdx.x;
  const int K = a.K, W = a.W;
  const int64_t r = a.dst ? (int64_t)a.dst[b] : a.base + b;
  const float* src = a.p + (int64_t)b * K * W;
  for (int w = wave; w < W; w += 4) {            // wave-uniform
    float f[MC_PER_LANE]; double d[MC_PER_LANE];
#pragma unroll
    for (int j = 0; j < MC_PER_LANE; ++j) {
      const int k = lane + 64 * j;
      f[j] = k < K ? src[(int64_t)k * W + w] : 0.f;
      d[j] = (double)f[j];
    }
    if (a.o.draws) {
      float* out = a.o.draws + r * K * W;
#pragma unroll
      for (int j = 0; j < MC_PER_LANE; ++j) {
        const int k = lane + 64 * j;
        if (k < K) out[(int64_t)k * W + w] = f[j];
      }
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < MC_PER_LANE; ++j) s += (lane + 64 * j < K) ? d[j] : 0.0;
    const double mean = wave_sum_widest_first(s) / (double)K;
    const int64_t at = r * W + w;
    if (a.o.mean && lane == 0) a.o.mean[at] = mean;
    if (a.o.var) {
      double q = 0.0;
#pragma unroll
      for (int j = 0; j < MC_PER_LANE; ++j) {
        const double e = d[j] - mean;
        q += (lane + 64 * j < K) ? e * e : 0.0;
      }
      const double var = wave_sum_widest_first(q) / (double)K;
      if (lane == 0) a.o.var[at] = var;
    }
    if (a.o.vote && a.thr) {
      const float t = a.thr[w];
      int c = 0;
#pragma unroll
      for (int j = 0; j < MC_PER_LANE; ++j) c += (lane + 64 * j < K && f[j] > t) ? 1 : 0;
      c = wave_sum_widest_first(c);
      if (lane == 0) a.o.vote[at] = (double)c / (double)K;       // the correctly rounded share (c * (1 / K) is an ulp off at K = 65)
    }
    if (a.bernoulli && (a.o.entropy || a.o.expected_entropy || a.o.mutual_info)) {
      double e = 0.0;
#pragma unroll
      for (int j = 0; j < MC_PER_LANE; ++j) e += (lane + 64 * j < K) ? bernoulli_entropy(d[j]) : 0.0;
      const double eh = wave_sum_widest_first(e) / (double)K;
      const double h = bernoulli_entropy(mean);
      const double diff = h - eh;
      const double mi = diff > 0.0 ? diff : (diff != diff ? diff : 0.0);       // max(0, .) that keeps a NaN
      if (lane == 0) {
        if (a.o.entropy) a.o.entropy[at] = h;
        if (a.o.expected_entropy) a.o.expected_entropy[at] = eh;
        if (a.o.mutual_info) a.o.mutual_info[at] = mi;
      }
    }
  }
}

}  // namespace

extern "C" int mmda_mc_reduce(const float* p, int B, int K, int W, const float* thr, int bernoulli, const mmda_mc_out* out,
                              const int32_t* dst, int64_t base, void* stream) {
  if (!p || !out) return MMDA_EINVAL;
  if (B < 1 || K < 1 || K > MC_MAX_K || W < 1 || W > MC_MAX_W) return MMDA_EINVAL;
  const bool entropy_tables = out->entropy || out->expected_entropy || out->mutual_info;
  if (entropy_tables && !bernoulli) return MMDA_EINVAL;
  // (the vote is skipped without thresholds: a vote table alone, without them, is nothing to write)
  if (!out->mean && !out->var && !entropy_tables && !(out->vote && thr) && !out->draws) return MMDA_EINVAL;
  McArgs a;
  a.p = p; a.thr = thr; a.o = *out; a.dst = dst; a.base = base; a.B = B; a.K = K; a.W = W; a.bernoulli = bernoulli ? 1 : 0;
  hipLaunchKernelGGL(mc_reduce_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  MMDA_CHECK_LAUNCH("mmda_mc_reduce");
  return MMDA_OK;
}

// The same on the model's own workspace: the B K columns of the last forward of the current carve, K adjacent columns per sample.
extern "C" int mmda_misa_mc_reduce(mmda_misa* m, int K, int which, const float* thr, const mmda_mc_out* out, const int32_t* dst,
                                   int64_t base, void* stream) {
  if (!m || !out || !m->ws || m->lay.B <= 0) return MMDA_EINVAL;
  if (which != 0 && which != 1) return MMDA_EINVAL;
  if (K < 1 || K > MC_MAX_K || m->lay.B % K != 0) return MMDA_EINVAL;
  const mmda_step::Workspace& w = m->lay;
  const float* p = m->ws + (which == 0 ? w.scores : w.tcp);
  // the entropy reads a score as a probability: the classifier's sigmoid scores only (not tcp, not a regression output)
  const int bernoulli = which == 0 && m->set.reg == REG_NONE;
  return mmda_mc_reduce(p, w.B / K, K, which == 0 ? m->cfg.ncls : 6, thr, bernoulli, out, dst, base, stream);
}
