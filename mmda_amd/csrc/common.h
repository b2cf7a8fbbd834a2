// Shared device/host helpers for the gfx950 kernels (wave64, MFMA fragment types, RNG, reductions).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/mmda_hip.h"

#define WAVE 64

typedef __attribute__((ext_vector_type(8))) short bf16x8;   // 8 bf16 = one 16x16x32 A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) float f32x4;     // 16x16 accumulator fragment

// Host: the environment switches of DESIGN §7a.  Callers keep the value in a function-local static, so each is read once per process.
static inline int mmda_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
static inline bool mmda_env_set(const char* name) { return getenv(name) != nullptr; }

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
// blocks of 256 lanes for a grid-stride loop over `work` items
static inline int stream_blocks(int64_t work) {
  const int64_t blocks = (work + 255) / 256;
  return (int)(blocks > 2048 ? 2048 : blocks < 1 ? 1 : blocks);
}

// fp32 -> bf16 round-to-nearest-even via the hardware cast (keeps NaN a NaN, MI355X_MICROARCH correctness table)
__device__ __forceinline__ unsigned short f2bf(float x) {
  __bf16 b = (__bf16)x;
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(unsigned short u) {
  return __builtin_bit_cast(float, ((unsigned)u) << 16);
}

// accurate versions (fp32 parity path and every non-recurrent kernel)
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// tanh via exp(-2|x|): saturates cleanly, |err| ~1e-7
__device__ __forceinline__ float tanhf_(float x) {
  float ax = fabsf(x);
  float e = expf(-2.0f * ax);
  float t = (1.0f - e) / (1.0f + e);
  return copysignf(t, x);
}
// fast versions (v_exp_f32 + v_rcp_f32) for the bf16 recurrent kernels where the gate math sits on the serial chain
// (__frcp_rn is a correctly rounded reciprocal = a ~10-instruction division sequence; v_rcp_f32 is 1 ulp and one issue)
__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_fast(float x) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)) - 1.0f; }

// Counter-based dropout RNG: murmur3 fmix64 of (seed, site, element index).  The same triple gives the same bit in
// forward and backward, so masks are never stored.
__device__ __forceinline__ uint32_t rng_u32(uint64_t seed, int site, uint64_t idx) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(site + 1) + idx * 0xD6E8FEB86659FD93ull;
  z ^= z >> 33; z *= 0xff51afd7ed558ccdull;
  z ^= z >> 33; z *= 0xc4ceb9fe1a85ec53ull;
  z ^= z >> 33;
  return (uint32_t)(z >> 16);
}
// inverted-dropout multiplier: 0 with probability p, else 1/(1-p)
__device__ __forceinline__ float drop_mul(float p, uint64_t seed, int site, uint64_t idx) {
  if (p <= 0.0f) return 1.0f;
  uint32_t r = rng_u32(seed, site, idx);
  float u = (float)(r >> 8) * (1.0f / 16777216.0f);
  return u < p ? 0.0f : 1.0f / (1.0f - p);
}

// Wave-wide sum / max, the same value in every lane.  Inside a row of 16 lanes by DPP (quad swaps, half-row mirror, row mirror: 4
// VALU instructions, every lane of a row ends with the row's result); the four rows are then read as scalars and combined.  (A
// __shfl_xor butterfly is six dependent ds_bpermute round trips, ~700 cycles: the 36 dot products of the six-token attention cost 11 us
// that way.)
#define MMDA_DPP(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), (ctrl), 0xf, 0xf, true))
__device__ __forceinline__ float wave_sum(float v) {
  v += MMDA_DPP(v, 0xB1);            // quad_perm [1,0,3,2]
  v += MMDA_DPP(v, 0x4E);            // quad_perm [2,3,0,1]
  v += MMDA_DPP(v, 0x141);           // row_half_mirror
  v += MMDA_DPP(v, 0x140);           // row_mirror
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
  return (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, MMDA_DPP(v, 0xB1));
  v = fmaxf(v, MMDA_DPP(v, 0x4E));
  v = fmaxf(v, MMDA_DPP(v, 0x141));
  v = fmaxf(v, MMDA_DPP(v, 0x140));
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
// block-wide sum for blockDim.x <= 1024 (multiple of 64); `red` is >= 16 floats of LDS. All threads get the result.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

__device__ __forceinline__ float act_fwd(int act, float x) {
  switch (act) {
    case MMDA_ACT_RELU: return x > 0.f ? x : 0.f;
    case MMDA_ACT_SIGMOID: return sigmoidf_(x);
    case MMDA_ACT_LEAKYRELU: return x > 0.f ? x : 0.01f * x;
    case MMDA_ACT_TANH: return tanhf_(x);
    case MMDA_ACT_ELU: return x > 0.f ? x : (__expf(x) - 1.0f);
    case MMDA_ACT_HARDTANH: return fminf(fmaxf(x, -1.f), 1.f);
    case MMDA_ACT_HARDSHRINK: return (x > 0.5f || x < -0.5f) ? x : 0.f;
    default: return x;
  }
}
// derivative w.r.t. the pre-activation x
__device__ __forceinline__ float act_bwd(int act, float x) {
  switch (act) {
    case MMDA_ACT_RELU: return x > 0.f ? 1.f : 0.f;
    case MMDA_ACT_SIGMOID: { float s = sigmoidf_(x); return s * (1.f - s); }
    case MMDA_ACT_LEAKYRELU: return x > 0.f ? 1.f : 0.01f;
    case MMDA_ACT_TANH: { float t = tanhf_(x); return 1.f - t * t; }
    case MMDA_ACT_ELU: return x > 0.f ? 1.f : __expf(x);
    case MMDA_ACT_HARDTANH: return (x > -1.f && x < 1.f) ? 1.f : 0.f;
    case MMDA_ACT_HARDSHRINK: return (x > 0.5f || x < -0.5f) ? 1.f : 0.f;
    default: return 1.f;
  }
}

// ---- parametrised activations (nn.PReLU / nn.RReLU of the reference's activation_dict, config.py:25-27)
__device__ __forceinline__ float act_slope_p(int act, const mmda_act_params& p, uint64_t idx) {
  if (act == MMDA_ACT_PRELU) return p.slope[0];
  if (!p.rand) return 0.5f * (p.lo + p.hi);
  const float u = (float)(rng_u32(p.seed, p.site, idx) >> 8) * (1.0f / 16777216.0f);
  return p.lo + (p.hi - p.lo) * u;
}
__device__ __forceinline__ bool act_is_p(int act) { return act == MMDA_ACT_PRELU || act == MMDA_ACT_RRELU; }
__device__ __forceinline__ float act_fwd_p(int act, float x, const mmda_act_params& p, uint64_t idx) {
  if (!act_is_p(act)) return act_fwd(act, x);
  return x > 0.f ? x : act_slope_p(act, p, idx) * x;
}
__device__ __forceinline__ float act_bwd_p(int act, float x, const mmda_act_params& p, uint64_t idx) {
  if (!act_is_p(act)) return act_bwd(act, x);
  return x > 0.f ? 1.f : act_slope_p(act, p, idx);
}

// ---- sparse update of the embedding table (embed_update = sparse): torch.optim.SparseAdam's rule on the rows a step touches, applied
// where a row's gradient sum becomes final (embed_rows.hip: the owning workgroup of the short form, the two levels of the sort form).
// P / M / V: the table and its two moments; step_size = lr sqrt(1 - b2^t) / (1 - b1^t), made on the host in double
// (mmda_sparse_adam_args); table_rows bounds the ids that are updated.
struct SparseAdamArgs { float* P; float* M; float* V; int table_rows; float b1, b2, eps, clip, gscale, step_size; };
// one element: g = clamp(gscale * sum, +-clip), then the update.  eps is added to sqrt(v) itself (SparseAdam), not to
// sqrt(v / (1 - b2^t)) as in the dense adam1() below.  Every rounding spelled out: both list paths give the same bits from
// the same sum.
__device__ __forceinline__ void sparse_adam1(float& p, float g, float& m, float& v, const SparseAdamArgs& a) {
  g = __fmul_rn(g, a.gscale);
  g = fminf(fmaxf(g, -a.clip), a.clip);
  m = __fmaf_rn(a.b1, m, __fmul_rn(1.f - a.b1, g));
  v = __fmaf_rn(a.b2, v, __fmul_rn(__fmul_rn(1.f - a.b2, g), g));
  p = __fmaf_rn(-a.step_size, __fdiv_rn(m, __fadd_rn(sqrtf(v), a.eps)), p);
}
// what the sums do with a finished row element: add it into the dense gradient, or update the table in place.  begin(): called by
// every thread of the launch that makes a row's first sums (the short form's one launch, level 1 of the sort form), before anything else
struct RowAdd {
  float* dW; int accumulate;
  __device__ __forceinline__ void begin() const {}
  __device__ __forceinline__ void operator()(int64_t id, int D, int c, float sum) const {
    float* dst = dW + id * D + c;                          // one writer per table row
    *dst = accumulate ? *dst + sum : sum;
  }
};
struct RowSparseAdam {
  SparseAdamArgs a;
  __device__ __forceinline__ void begin() const {}
  __device__ __forceinline__ void operator()(int64_t id, int D, int c, float sum) const {
    const int64_t o = id * D + c;                          // one writer per table row
    float p = a.P[o], m = a.M[o], v = a.V[o];
    sparse_adam1(p, sum, m, v, a);
    a.P[o] = p; a.M[o] = m; a.V[o] = v;
  }
};
// ---- dense Adam, one element (optim.hip: the Adam functors under every walker; embed_rows.hip: the deferred table update below)
// moments and update from a gradient that is already scaled, clamped (and, under L2 decay, decayed)
__device__ __forceinline__ void adam1_update(float& p, float g, float& m, float& v, float b1, float b2, float eps, float step_size,
                                             float inv_bc2_sqrt) {
  m = __fmaf_rn(b1, m, __fmul_rn(1.f - b1, g));
  v = __fmaf_rn(b2, v, __fmul_rn(__fmul_rn(1.f - b2, g), g));
  const float denom = __fmaf_rn(sqrtf(v), inv_bc2_sqrt, eps);
  p = __fmaf_rn(-step_size, __fdiv_rn(m, denom), p);
}
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float b1, float b2, float eps, float clip,
                                      float gscale, float step_size, float inv_bc2_sqrt) {
  // every rounding spelled out: the dense kernel and the per-row kernel below must give the same bits (the fused step runs part of the
  // bucket through each), whatever the compiler would contract in either loop
  g = __fmul_rn(g, gscale);
  g = fminf(fmaxf(g, -clip), clip);
  adam1_update(p, g, m, v, b1, b2, eps, step_size, inv_bc2_sqrt);
}
// Adam with weight decay.  decay: MMDA_DECAY_L2 (torch.optim.Adam(weight_decay = wd)): the scaled, clamped gradient takes wd p in one
// fma and everything follows from that; MMDA_DECAY_DECOUPLED (torch.optim.AdamW): p <- p - (lr wd) p in one fma first, then adam1's
// moments and update on the decayed p (lr_wd = lr wd, made on the host in double and rounded once, like step_size); anything else:
// adam1.  Launch-uniform.
enum { MMDA_DECAY_NONE = 0, MMDA_DECAY_L2 = 1, MMDA_DECAY_DECOUPLED = 2 };
__device__ __forceinline__ void adam1_decayed(float& p, float g, float& m, float& v, float b1, float b2, float eps, float clip,
                                              float gscale, float step_size, float inv_bc2_sqrt, int decay, float wd, float lr_wd) {
  g = __fmul_rn(g, gscale);
  g = fminf(fmaxf(g, -clip), clip);
  if (decay == MMDA_DECAY_L2) g = __fmaf_rn(wd, p, g);
  else if (decay == MMDA_DECAY_DECOUPLED) p = __fmaf_rn(-lr_wd, p, p);
  adam1_update(p, g, m, v, b1, b2, eps, step_size, inv_bc2_sqrt);
}

// Wave-wide sum of doubles in a fixed order, the same value in every lane: an xor butterfly (a double has no DPP add; the six round
// trips are paid once per workgroup of a streaming reduction, where they do not show).
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
// The same butterfly with the widest step first (32 .. 1), doubles or integers.  Two orders exist because results are pinned to each:
// the Jaccard sum of the evaluation counts and the MC-dropout tables to 32 .. 1, the streaming reductions above to 1 .. 32.
template <typename T>
__device__ __forceinline__ T wave_sum_widest_first(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- deferred dense update of the embedding table (embed_update = deferred): dense Adam's result, without a pass over the table.  A row
// whose gradient is zero takes a step that needs nothing but the row and the step's two scalars, so it can be applied later.  Updates are
// counted as they are applied, 1, 2, 3 ... since the state was reset (`seq`; the Adam step NUMBER t that makes the bias corrections is
// the caller's and may skip): row_step[id] is the count of the last update row id has taken, and ring[2 (s % window)],
// ring[2 (s % window) + 1] keep update s's step_size = lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) -- the floats the dense launch of that
// update is given -- for the last `window` updates.  A stale row is replayed with adam1(g = 0) update by update (embed_rows.hip), a row of
// the batch takes update `seq` here, where its sum becomes final, with the sum the dense scatter would have added into a cleared
// gradient row.
struct DenseRowArgs {
  float* P; float* M; float* V; int* row_step; float* ring; int window; int table_rows;
  float b1, b2, eps, clip, gscale, step_size, inv_bc2_sqrt; int seq;
};
// the launch that applies update `seq` also records its scalars (its first thread; the launches that replay it come later on the stream)
__device__ __forceinline__ void dense_row_record(const DenseRowArgs& a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.ring[2 * (a.seq % a.window)] = a.step_size;
    a.ring[2 * (a.seq % a.window) + 1] = a.inv_bc2_sqrt;
  }
}
// requires row id current at seq - 1 (every forward catches the batch's rows up); 0 + sum: what `+=` into the cleared row leaves
struct RowDenseAdam {
  DenseRowArgs a;
  __device__ __forceinline__ void begin() const { dense_row_record(a); }
  __device__ __forceinline__ void operator()(int64_t id, int D, int c, float sum) const {
    const int64_t o = id * D + c;                          // one writer per table row
    float p = a.P[o], m = a.M[o], v = a.V[o];
    adam1(p, __fadd_rn(0.f, sum), m, v, a.b1, a.b2, a.eps, a.clip, a.gscale, a.step_size, a.inv_bc2_sqrt);
    a.P[o] = p; a.M[o] = m; a.V[o] = v;
    if (c == 0) a.row_step[id] = a.seq;
  }
};

// ---- flag joins (misa_streams.hip: side_flag_signal): a kernel of one stream waits, on the device, for a word that a one-thread launch behind
// the last kernel of ANOTHER stream's chain sets to `value` -- instead of a stream-level event wait, which costs the waiting stream
// 9 - 12 us of packet processing however early the other chain finished (tools/micro/fork_cost.hip).  Called by every thread of the
// workgroup; thread 0 polls (bounded: a word that never arrives is reported through *err and the kernel goes on), a workgroup
// barrier and an agent-scope acquire follow.  flag == nullptr: nothing to wait for (workgroup-uniform).
__device__ __forceinline__ void flag_wait(const unsigned* flag, unsigned value, unsigned* err) {
  if (!flag) return;
  if (threadIdx.x == 0) {
    int polls = 0;
    while ((int)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - value) < 0) {
      __builtin_amdgcn_s_sleep(16);
      if (++polls > (1 << 21)) { if (err) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

