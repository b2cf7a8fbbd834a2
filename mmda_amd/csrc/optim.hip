// clip_grad_value_ + the optimizer's update fused over flat fp32 buckets.  The reference builds torch.optim.Adam with lr only
// (solver.py:97-99: betas (0.9, 0.999), eps 1e-8, no weight decay), and that is what launches by default; betas and eps are arguments
// of every launch, weight decay (L2 as torch.optim.Adam's, decoupled as torch.optim.AdamW's) and a gradient scale read from device
// memory (clip_grad_norm_'s coefficient) come with mmda_adam_opts.  An update rule is an element functor, a memory layout is a walker
// kernel that takes one; a launch is a walker instantiated with a rule.  Also here: the gradient's global L2 norm (grad_norm_kernel)
// and its in-place scaling (the Scale functor).
#include "common.h"
#include "internal.h"
#include <math.h>
#include <type_traits>

// ---- Adam's bias corrections and step scalars (internal.h: the rows code of embed_rows.hip makes its scalars from the same two)
BiasCorrections bias_corrections(float beta1, float beta2, int step) {
  return {1.0 - pow((double)beta1, (double)step), 1.0 - pow((double)beta2, (double)step)};
}
AdamStepScalars adam_step_scalars(float lr, float beta1, float beta2, int step) {
  const BiasCorrections c = bias_corrections(beta1, beta2, step);
  return {(float)((double)lr / c.bc1), (float)(1.0 / sqrt(c.bc2))};
}

namespace {

// ---- the update rules: one element functor per rule
// quad(q): the rule over floats 4 q .. 4 q + 3 of the flat buffers, with 16-byte accesses (every base is 16-byte aligned); one(e): over
// float e.  Which quads and floats a launch takes is the walker's business (below), so every launch of a rule gives an element the same
// bits, whatever layout it is reached through.
// clip_grad_value_ + Adam (adam1(), common.h).  kSum: the gradient is acc + g, one IEEE add -- the closing step of an accumulated update
// reads the last micro-batch's gradients where the backward pass left them, instead of adding them into the accumulator first and
// reading that back: the bits of "accumulate, then Adam over the accumulator".  Neither acc nor g is written.
struct AdamArgs { float* p; const float* acc; const float* g; float* m; float* v; float b1, b2, eps, clip, gscale, step_size, inv_bc2_sqrt; };
template <bool kSum>
struct Adam : AdamArgs {
  __device__ __forceinline__ void step4(float4& pp, const float4& gg, float4& mm, float4& vv) const {
    adam1(pp.x, gg.x, mm.x, vv.x, b1, b2, eps, clip, gscale, step_size, inv_bc2_sqrt);
    adam1(pp.y, gg.y, mm.y, vv.y, b1, b2, eps, clip, gscale, step_size, inv_bc2_sqrt);
    adam1(pp.z, gg.z, mm.z, vv.z, b1, b2, eps, clip, gscale, step_size, inv_bc2_sqrt);
    adam1(pp.w, gg.w, mm.w, vv.w, b1, b2, eps, clip, gscale, step_size, inv_bc2_sqrt);
  }
  __device__ __forceinline__ void quad(int64_t q) const {
    float4 pp = reinterpret_cast<float4*>(p)[q], mm = reinterpret_cast<float4*>(m)[q], vv = reinterpret_cast<float4*>(v)[q];
    float4 gg = reinterpret_cast<const float4*>(g)[q];
    if constexpr (kSum) {
      const float4 aa = reinterpret_cast<const float4*>(acc)[q];
      gg.x = __fadd_rn(aa.x, gg.x); gg.y = __fadd_rn(aa.y, gg.y); gg.z = __fadd_rn(aa.z, gg.z); gg.w = __fadd_rn(aa.w, gg.w);
    }
    step4(pp, gg, mm, vv);
    reinterpret_cast<float4*>(p)[q] = pp; reinterpret_cast<float4*>(m)[q] = mm; reinterpret_cast<float4*>(v)[q] = vv;
  }
  __device__ __forceinline__ void one(int64_t e) const {
    float ge = g[e];
    if constexpr (kSum) ge = __fadd_rn(acc[e], ge);
    adam1(p[e], ge, m[e], v[e], b1, b2, eps, clip, gscale, step_size, inv_bc2_sqrt);
  }
  // the step of an element whose gradient is gz, a zero the launch is handed at run time (background_kernel below): g is not read
  __device__ __forceinline__ void one_zero(float& pe, float& me, float& ve, float gz) const {
    adam1(pe, gz, me, ve, b1, b2, eps, clip, gscale, step_size, inv_bc2_sqrt);
  }
};
// Adam with what mmda_adam_opts adds: weight decay (adam1_decayed(), common.h) and a gradient scale that lives on the device -- the
// coefficient grad_norm_finish_kernel wrote, never read by the host: gscale * *scale_dev, rounded once, takes gscale's place (with
// gscale = 1 that is torch's g.mul_(clip_coef)).  The decay kind is a launch-uniform branch, not a template parameter: one scalar
// compare per element beside 28 B of HBM traffic, against three times the instances under three walkers.  Launches with no decay and
// no device scale keep the Adam<> instances above.
struct AdamOptArgs : AdamArgs { int decay; float wd, lr_wd; const float* scale_dev; };
template <bool kSum>
struct AdamOpt : AdamOptArgs {
  __device__ __forceinline__ float scale() const { return scale_dev ? __fmul_rn(gscale, *scale_dev) : gscale; }
  __device__ __forceinline__ void step4(float4& pp, const float4& gg, float4& mm, float4& vv, float gs) const {
    adam1_decayed(pp.x, gg.x, mm.x, vv.x, b1, b2, eps, clip, gs, step_size, inv_bc2_sqrt, decay, wd, lr_wd);
    adam1_decayed(pp.y, gg.y, mm.y, vv.y, b1, b2, eps, clip, gs, step_size, inv_bc2_sqrt, decay, wd, lr_wd);
    adam1_decayed(pp.z, gg.z, mm.z, vv.z, b1, b2, eps, clip, gs, step_size, inv_bc2_sqrt, decay, wd, lr_wd);
    adam1_decayed(pp.w, gg.w, mm.w, vv.w, b1, b2, eps, clip, gs, step_size, inv_bc2_sqrt, decay, wd, lr_wd);
  }
  __device__ __forceinline__ void quad(int64_t q) const {
    const float gs = scale();
    float4 pp = reinterpret_cast<float4*>(p)[q], mm = reinterpret_cast<float4*>(m)[q], vv = reinterpret_cast<float4*>(v)[q];
    float4 gg = reinterpret_cast<const float4*>(g)[q];
    if constexpr (kSum) {
      const float4 aa = reinterpret_cast<const float4*>(acc)[q];
      gg.x = __fadd_rn(aa.x, gg.x); gg.y = __fadd_rn(aa.y, gg.y); gg.z = __fadd_rn(aa.z, gg.z); gg.w = __fadd_rn(aa.w, gg.w);
    }
    step4(pp, gg, mm, vv, gs);
    reinterpret_cast<float4*>(p)[q] = pp; reinterpret_cast<float4*>(m)[q] = mm; reinterpret_cast<float4*>(v)[q] = vv;
  }
  __device__ __forceinline__ void one(int64_t e) const {
    float ge = g[e];
    if constexpr (kSum) ge = __fadd_rn(acc[e], ge);
    adam1_decayed(p[e], ge, m[e], v[e], b1, b2, eps, clip, scale(), step_size, inv_bc2_sqrt, decay, wd, lr_wd);
  }
  __device__ __forceinline__ void one_zero(float& pe, float& me, float& ve, float gz) const {
    adam1_decayed(pe, gz, me, ve, b1, b2, eps, clip, scale(), step_size, inv_bc2_sqrt, decay, wd, lr_wd);
  }
};
// g *= *scale_dev in place: clip_grad_norm_'s second half for the unfused loop
struct Scale {
  float* g; const float* scale_dev;
  __device__ __forceinline__ void quad(int64_t q) const {
    const float s = *scale_dev;
    float4 gg = reinterpret_cast<float4*>(g)[q];
    gg.x = __fmul_rn(gg.x, s); gg.y = __fmul_rn(gg.y, s); gg.z = __fmul_rn(gg.z, s); gg.w = __fmul_rn(gg.w, s);
    reinterpret_cast<float4*>(g)[q] = gg;
  }
  __device__ __forceinline__ void one(int64_t e) const { g[e] = __fmul_rn(g[e], *scale_dev); }
};
struct RunRmsprop {         // clamp_rmsprop_kernel's (below: the dense launch keeps its one-float-per-lane loop)
  float* p; const float* g; float* sq; float lr, alpha, eps, clip, gscale;
  // That kernel leaves contraction to the compiler, which forms no fma in its loop; the same statements unrolled over a quad here did
  // get one (alpha * sq + ...) and lost the dense launch's bits.  So: the operations its code performs, in its order, with contraction
  // off for this block -- on plain operators: __fadd_rn / __fmul_rn are functions of a header compiled with contraction on, and what
  // they return is fused all the same.  tests/test_gpu_frozen.py holds the two launches together.
  __device__ __forceinline__ void one(int64_t i) const {
#pragma clang fp contract(off)
    const float gg = fminf(fmaxf(g[i] * gscale, -clip), clip);
    const float old = alpha * sq[i];
    const float add = ((1.0f - alpha) * gg) * gg;
    const float s = old + add;
    sq[i] = s;
    const float num = lr * gg;
    const float den = sqrtf(s) + eps;
    p[i] = p[i] - num / den;
  }
  __device__ __forceinline__ void quad(int64_t q) const {
    for (int k = 0; k < 4; ++k) one((q << 2) + k);
  }
};

// ---- the walkers: one per memory layout
// Dense stream over n floats: 16 bytes per lane, a scalar tail.  Pure HBM traffic (Adam: reads p, g, m, v and writes p, m, v = 28 B per
// parameter).  wait_flag != nullptr (flag join, common.h): workgroup 0 does not finish before that word reaches wait_value -- so the
// completion of this launch on its stream implies the completion of the other stream's chain (the update itself does not depend on it).
template <class F>
__global__ __launch_bounds__(256) void stream_kernel(int64_t n, F f, const unsigned* wait_flag, unsigned wait_value, unsigned* wait_err) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += stride) f.quad(i);
  for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) f.one(i);
  if (blockIdx.x == 0) flag_wait(wait_flag, wait_value, wait_err);
}

// The ROWS of a (rows, dim) table whose mask byte equals `want`; vec: dim % 4 == 0 and 16-byte aligned bases, so every row is whole quads
// (launch-uniform).  The embedding matrix is 6 of the model's 10.8 M parameters and a step touches at most T*B of its V rows: the rows a
// batch does not touch have a zero gradient that is known before the backward pass ends, so their update runs early, beside the last
// recurrence (mask 0), and only the touched rows wait for the scattered gradient (mask 1).  One wave per row, lanes along the row.
template <class F>
__global__ __launch_bounds__(256) void rows_kernel(int rows, int dim, const unsigned char* __restrict__ mask, int want, int vec, F f) {
  const int lane = threadIdx.x & 63;
  const int wpg = (int)gridDim.x * 4;
  for (int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += wpg) {
    if ((int)mask[row] != want) continue;                // wave-uniform
    const int64_t o = (int64_t)row * dim;
    if (vec) for (int i = lane; i < (dim >> 2); i += 64) f.quad((o >> 2) + i);
    else for (int i = lane; i < dim; i += 64) f.one(o + i);
  }
}

// The TRAINABLE RUNS of a bucket (frozen parameters, requires_grad = False; mmda_hip.h: mmda_run).
// A work item is one 16-byte aligned quad of the bucket that a run touches; the grid is sized by the items, and item j of the launch
// finds its run by bisection over the runs' running counts (a few hundred entries at the most, read by every lane: they stay in
// cache).  A quad that lies inside its run goes through quad() like the dense stream's; a quad at a run's end takes the floats of the
// run one by one, so no float outside a run is loaded or stored -- two runs that share a quad touch disjoint floats of it.  wait_flag:
// as in stream_kernel (the same flag_wait).
struct RunItem { int64_t q, e0, e1; };                          // the bucket's quad, and the floats [e0, e1) of it that the run holds
__device__ __forceinline__ RunItem run_item(const mmda_run* __restrict__ runs, int n_runs, int64_t j) {
  int lo = 0, hi = n_runs - 1;                                     // the last run whose count is <= j
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (runs[mid].first <= j) lo = mid; else hi = mid - 1;
  }
  const mmda_run r = runs[lo];
  const int64_t q = (r.begin >> 2) + (j - r.first);
  return {q, max(q << 2, r.begin), min((q << 2) + 4, r.begin + r.len)};
}
template <class F>
__global__ __launch_bounds__(256) void runs_kernel(const mmda_run* __restrict__ runs, int n_runs, int64_t items, F f,
                                                   const unsigned* wait_flag, unsigned wait_value, unsigned* wait_err) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t item0 = n_runs > 0 ? runs[0].first : 0;          // (a slice of a longer table: counts run on from its start)
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += stride) {
    const RunItem it = run_item(runs, n_runs, item0 + i);
    if (it.e1 - it.e0 == 4) f.quad(it.q);
    else for (int64_t e = it.e0; e < it.e1; ++e) f.one(e);
  }
  if (blockIdx.x == 0) flag_wait(wait_flag, wait_value, wait_err);
}

// The embedding table BY STAMP (internal.h: TableRows): row r is one the step's batch indexes when stamp[r] == epoch.  Both kernels walk
// the table flat -- item i is quad i of the table (vec: dim % 4 == 0 and 16-byte aligned bases, launch-uniform) or float i, its row
// i / (dim / 4) or i / dim; fewer than 2^31 items, so the index arithmetic is 32-bit -- and consecutive lanes take consecutive items, so
// a wave's accesses are whole lines whichever rows it skips.
//
// The step's closing launch: the dense stream over [0, n) as stream_kernel walks it, then the rows of the table at float `off` that the
// batch indexes, through the same quad() / one() -- they read the scattered gradient.  The other rows took the step already
// (background_kernel).  wait_flag: as in stream_kernel.
template <class F>
__global__ __launch_bounds__(256) void stream_table_kernel(int64_t n, int64_t off, TableRows t, int vec, F f, const unsigned* wait_flag,
                                                           unsigned wait_value, unsigned* wait_err) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = i0; i < n4; i += stride) f.quad(i);
  for (int64_t i = (n4 << 2) + i0; i < n; i += stride) f.one(i);
  const unsigned per_row = vec ? (unsigned)t.dim >> 2 : (unsigned)t.dim;
  const int64_t items = (int64_t)t.rows * per_row;
  for (int64_t i = i0; i < items; i += stride) {
    if (t.stamp[(unsigned)i / per_row] != t.epoch) continue;
    if (vec) f.quad((off >> 2) + i);
    else f.one(off + i);
  }
  if (blockIdx.x == 0) flag_wait(wait_flag, wait_value, wait_err);
}

// The background pass: the rows the batch does NOT index take the step with the gradient gz -- a zero handed over at run time, so the
// functor's arithmetic is compiled as it is for a gradient read from memory, signed zeros included; g is not read.  f's p, m, v are the
// table's own.  A few workgroups (the launch's grid is its throttle) stream the table with non-temporal accesses beside the step's
// latency-bound kernels: four items per lane in flight, loads first.  No atomics, no waiting.  The launch may ask for LDS it never
// touches: a resident recurrence reserves the whole LDS of the CUs it runs on, so a workgroup that holds any is placed on another CU
// and does not queue its 16-byte accesses in front of a recurrence wave's hand-off loads in that CU's vector memory path.
template <class F>
__global__ __launch_bounds__(256) void background_kernel(TableRows t, int vec, F f, float gz) {
  const unsigned stride = gridDim.x * blockDim.x;
  const unsigned per_row = vec ? (unsigned)t.dim >> 2 : (unsigned)t.dim;
  const unsigned items = (unsigned)t.rows * per_row;
  if (vec) {
    f32x4* const P4 = reinterpret_cast<f32x4*>(f.p); f32x4* const M4 = reinterpret_cast<f32x4*>(f.m); f32x4* const V4 = reinterpret_cast<f32x4*>(f.v);
    for (unsigned base = blockIdx.x * blockDim.x + threadIdx.x; base < items; base += 4u * stride) {
      // (base + k stride < 2^31 + 4 * 2^20: no wrap -- the launcher caps the grid at 4096 workgroups)
      bool on[4]; f32x4 pp[4], mm[4], vv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned i = base + (unsigned)k * stride;
        on[k] = i < items && t.stamp[min(i, items - 1u) / per_row] != t.epoch;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned i = base + (unsigned)k * stride;
        if (on[k]) { pp[k] = __builtin_nontemporal_load(P4 + i); mm[k] = __builtin_nontemporal_load(M4 + i); vv[k] = __builtin_nontemporal_load(V4 + i); }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned i = base + (unsigned)k * stride;
        if (!on[k]) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) { float pe = pp[k][c], me = mm[k][c], ve = vv[k][c]; f.one_zero(pe, me, ve, gz); pp[k][c] = pe; mm[k][c] = me; vv[k][c] = ve; }
        __builtin_nontemporal_store(pp[k], P4 + i); __builtin_nontemporal_store(mm[k], M4 + i); __builtin_nontemporal_store(vv[k], V4 + i);
      }
    }
    return;
  }
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
    if (t.stamp[i / per_row] == t.epoch) continue;
    float pe = __builtin_nontemporal_load(f.p + i), me = __builtin_nontemporal_load(f.m + i), ve = __builtin_nontemporal_load(f.v + i);
    f.one_zero(pe, me, ve, gz);
    __builtin_nontemporal_store(pe, f.p + i); __builtin_nontemporal_store(me, f.m + i); __builtin_nontemporal_store(ve, f.v + i);
  }
}

// ---- the global L2 norm of the gradient a step is about to apply (torch.nn.utils.clip_grad_norm_)
// The gradient is g, or acc + g with the one IEEE add the Adam functors make (kSum).  runs == nullptr: the dense range [0, n) in
// stream_kernel's order, 16 bytes per lane and a scalar tail; otherwise the items of a run table with runs_kernel's mapping, so no float
// outside a run is loaded (a frozen tensor's gradient slot may hold anything).  The squares are summed in double -- the product of two
// floats is exact there -- by each lane over its grid-stride items, then in a fixed order inside the wave and across the block's four
// waves; block b leaves its sum in partials[b].  No atomics: two launches give equal bits.
template <bool kSum>
__global__ __launch_bounds__(256) void grad_norm_kernel(const float* __restrict__ acc, const float* __restrict__ g, int64_t n,
                                                        const mmda_run* __restrict__ runs, int n_runs, int64_t items,
                                                        double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  double s = 0.0;
  auto one = [&](int64_t e) {
    float ge = g[e];
    if constexpr (kSum) ge = __fadd_rn(acc[e], ge);
    s += (double)ge * (double)ge;
  };
  auto quad = [&](int64_t q) {
    float4 gg = reinterpret_cast<const float4*>(g)[q];
    if constexpr (kSum) {
      const float4 aa = reinterpret_cast<const float4*>(acc)[q];
      gg.x = __fadd_rn(aa.x, gg.x); gg.y = __fadd_rn(aa.y, gg.y); gg.z = __fadd_rn(aa.z, gg.z); gg.w = __fadd_rn(aa.w, gg.w);
    }
    s += (double)gg.x * (double)gg.x; s += (double)gg.y * (double)gg.y; s += (double)gg.z * (double)gg.z; s += (double)gg.w * (double)gg.w;
  };
  if (!runs) {                                                     // launch-uniform
    const int64_t n4 = n >> 2;
    for (int64_t i = i0; i < n4; i += stride) quad(i);
    for (int64_t i = (n4 << 2) + i0; i < n; i += stride) one(i);
  } else {
    const int64_t item0 = n_runs > 0 ? runs[0].first : 0;
    for (int64_t i = i0; i < items; i += stride) {
      const RunItem it = run_item(runs, n_runs, item0 + i);
      if (it.e1 - it.e0 == 4) quad(it.q);
      else for (int64_t e = it.e0; e < it.e1; ++e) one(e);
    }
  }
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
// One wave behind it on the stream: lane l adds the partials [l c, (l + 1) c) in block-index order, the 64 lane sums meet in the fixed
// order of the butterfly.  out[0] = norm = (float)(gscale sqrt(sum)), out[1] = coef = min(1, max_norm / (norm + 1e-6)) in fp32:
// clip_grad_norm_'s two expressions.  nb == 0 (nothing trains): norm 0, coef 1.
__global__ __launch_bounds__(64) void grad_norm_finish_kernel(const double* __restrict__ partials, int nb, float gscale, float max_norm,
                                                              float* __restrict__ out) {
  const int c = (nb + 63) >> 6;
  double s = 0.0;
  for (int i = threadIdx.x * c; i < min((int)(threadIdx.x + 1) * c, nb); ++i) s += partials[i];
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) {
    const float norm = (float)((double)gscale * sqrt(s));
    out[0] = norm;
    out[1] = fminf(1.f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f)));
  }
}

// ---- gradient accumulation (accum_steps > 1): one optimizer step from the gradients of several micro-batches
// acc = g (first: a plain copy, so the accumulator never needs clearing) or acc = acc + g, one IEEE add per element.  Pure HBM stream:
// float4 per lane, scalar tail, the shape of stream_kernel.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* acc, const float* __restrict__ g, int64_t n, int first) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float4* a4 = reinterpret_cast<float4*>(acc);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  if (first) {                                             // launch-uniform
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += stride) a4[i] = g4[i];
    for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) acc[i] = g[i];
    return;
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 aa = a4[i];
    const float4 gg = g4[i];
    aa.x = __fadd_rn(aa.x, gg.x); aa.y = __fadd_rn(aa.y, gg.y); aa.z = __fadd_rn(aa.z, gg.z); aa.w = __fadd_rn(aa.w, gg.w);
    a4[i] = aa;
  }
  for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) acc[i] = __fadd_rn(acc[i], g[i]);
}


__global__ void mark_rows_kernel(unsigned char* mask, int rows, const int64_t* __restrict__ ids, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t id = ids[i];
  if (id >= 0 && id < rows) mask[id] = 1;
}

// clip_grad_value_ + torch.optim.RMSprop (alpha, eps; no momentum, not centered, no weight decay: the reference constructs its
// optimizer as config.optimizer(params, lr=...), solver.py:97-99, so every other argument is torch's default)
__global__ __launch_bounds__(256) void clamp_rmsprop_kernel(float* p, const float* __restrict__ g, float* sq, int64_t n, float lr,
                                                            float alpha, float eps, float clip, float gscale) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gg = fminf(fmaxf(g[i] * gscale, -clip), clip);
    const float s = alpha * sq[i] + (1.0f - alpha) * gg * gg;
    sq[i] = s;
    p[i] -= lr * gg / (sqrtf(s) + eps);
  }
}

// two buffers cleared by one launch (16-byte stores; counts in floats, multiples of 4, 16-byte aligned bases)
__global__ __launch_bounds__(256) void zero2_kernel(float4* a, int64_t na4, float4* b, int64_t nb4) {
  const float4 z = {0.f, 0.f, 0.f, 0.f};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < na4 + nb4; i += stride) {
    if (i < na4) a[i] = z;
    else b[i - na4] = z;
  }
}

__global__ void clamp_kernel(float* g, int64_t n, float clip) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    g[i] = fminf(fmaxf(g[i], -clip), clip);
}

// ---- host side: what every launcher below shares
AdamArgs adam_args(float* p, const float* acc, const float* g, float* m, float* v, const AdamHyper& h) {
  const AdamStepScalars s = adam_step_scalars(h.lr, h.beta1, h.beta2, h.step);
  return {p, acc, g, m, v, h.beta1, h.beta2, h.eps, h.clip, h.grad_scale, s.step_size, s.inv_bc2_sqrt};
}

// the decay kind a launch runs with, and lr wd in double, rounded once
AdamOptArgs adam_opt_args(const AdamArgs& a, const AdamHyper& h) {
  const int decay = h.weight_decay > 0.f ? (h.decoupled ? MMDA_DECAY_DECOUPLED : MMDA_DECAY_L2) : MMDA_DECAY_NONE;
  return {a, decay, h.weight_decay, (float)((double)h.lr * (double)h.weight_decay), h.scale_dev};
}
bool adam_plain(const AdamHyper& h) { return !(h.weight_decay > 0.f) && !h.scale_dev; }
bool adam_opts_ok(const mmda_adam_opts* o) {
  return o && o->beta1 >= 0.f && o->beta1 < 1.f && o->beta2 >= 0.f && o->beta2 < 1.f && o->eps >= 0.f && o->weight_decay >= 0.f;
}
AdamHyper adam_hyper(float lr, float clip, float grad_scale, int step, const mmda_adam_opts& o) {
  return {lr, o.beta1, o.beta2, o.eps, clip, grad_scale, step, o.weight_decay, o.decoupled, o.scale_dev};
}

template <class F>
int launch_stream(const char* what, int64_t n, const F& f, const FlagWait& w, void* stream) {
  hipLaunchKernelGGL(stream_kernel<F>, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, n, f, w.flag, w.value, w.err);
  MMDA_CHECK_LAUNCH(what);
  return MMDA_OK;
}
template <class F>
int launch_runs(const char* what, const RunTable& t, const F& f, const FlagWait& w, void* stream) {
  hipLaunchKernelGGL(runs_kernel<F>, dim3(stream_blocks(t.items)), dim3(256), 0, (hipStream_t)stream, t.runs, t.n_runs, t.items, f, w.flag,
                     w.value, w.err);
  MMDA_CHECK_LAUNCH(what);
  return MMDA_OK;
}

}  // namespace

// internal.h: the launch behind every mmda_clamp_adam* entry (and misa_step.hip's).  A waiter with nothing to update gets the dense stream
// over no floats.
int mmda_adam_launch(float* p, const float* acc, const float* g, float* m, float* v, int64_t n, const RunTable* table, const AdamHyper& h,
                     const FlagWait& w, void* stream) {
  if (!p || !g || !m || !v || h.step < 1) return MMDA_EINVAL;
  if (table ? (table->n_runs < 0 || table->items < 0) : n < 0) return MMDA_EINVAL;
  if (((uintptr_t)p | (uintptr_t)acc | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return MMDA_EINVAL;   // 16-byte quads
  const bool empty = table ? (table->n_runs == 0 || table->items == 0) : n == 0;
  if (empty && !w.flag) return MMDA_OK;
  if (table && !empty && !table->runs) return MMDA_EINVAL;
  const char* what = table ? (acc ? "mmda_clamp_adam_sum_runs" : "mmda_clamp_adam_runs") : (acc ? "mmda_clamp_adam_sum" : "mmda_clamp_adam");
  const AdamArgs a = adam_args(p, acc, g, m, v, h);
  auto launch = [&](const auto& f) {
    return table && !empty ? launch_runs(what, *table, f, w, stream) : launch_stream(what, empty ? 0 : n, f, w, stream);
  };
  if (adam_plain(h)) return acc ? launch(Adam<true>{a}) : launch(Adam<false>{a});
  const AdamOptArgs o = adam_opt_args(a, h);
  return acc ? launch(AdamOpt<true>{o}) : launch(AdamOpt<false>{o});
}

// internal.h: the two launches of a step whose table is walked by stamp
bool mmda_table_rows_ok(const TableRows& t) {
  return t.stamp && t.rows > 0 && t.dim > 0 && (int64_t)t.rows * t.dim < ((int64_t)1 << 31);
}
int mmda_adam_tail_launch(float* p, const float* g, float* m, float* v, int64_t n, const TableRows& t, const AdamHyper& h, const FlagWait& w,
                          void* stream) {
  if (!p || !g || !m || !v || h.step < 1 || n < 0 || !mmda_table_rows_ok(t)) return MMDA_EINVAL;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return MMDA_EINVAL;
  const int vec = (n & 3) == 0 && (t.dim & 3) == 0;
  const int64_t items = (int64_t)t.rows * (vec ? t.dim >> 2 : t.dim);
  const int blocks = stream_blocks(items > n / 4 ? items : n / 4);
  const AdamArgs a = adam_args(p, nullptr, g, m, v, h);
  auto launch = [&](const auto& f) {
    using F = std::decay_t<decltype(f)>;
    hipLaunchKernelGGL(stream_table_kernel<F>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, n, t, vec, f, w.flag, w.value, w.err);
    MMDA_CHECK_LAUNCH("mmda_clamp_adam/table_tail");
    return (int)MMDA_OK;
  };
  if (adam_plain(h)) return launch(Adam<false>{a});
  return launch(AdamOpt<false>{adam_opt_args(a, h)});
}
int mmda_adam_background_launch(float* p, float* m, float* v, const TableRows& t, const AdamHyper& h, int workgroups, int lds_bytes,
                                void* stream) {
  if (!p || !m || !v || h.step < 1 || h.scale_dev || workgroups < 1 || workgroups > 4096 || !mmda_table_rows_ok(t)) return MMDA_EINVAL;
  if (lds_bytes < 0 || lds_bytes > 65536) return MMDA_EINVAL;
  if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 3) return MMDA_EINVAL;
  const int vec = (t.dim & 3) == 0 && (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  const AdamArgs a = adam_args(p, nullptr, nullptr, m, v, h);
  const float gz = 0.0f;
  auto launch = [&](const auto& f) {
    using F = std::decay_t<decltype(f)>;
    hipLaunchKernelGGL(background_kernel<F>, dim3(workgroups), dim3(256), (size_t)lds_bytes, (hipStream_t)stream, t, vec, f, gz);
    MMDA_CHECK_LAUNCH("mmda_clamp_adam/table_background");
    return (int)MMDA_OK;
  };
  if (adam_plain(h)) return launch(Adam<false>{a});
  return launch(AdamOpt<false>{adam_opt_args(a, h)});
}

bool mmda_adam_opts_valid(const mmda_adam_opts* o) { return adam_opts_ok(o); }

// what mmda_clamp_adam, _sum, _runs and _sum_runs cover, with mmda_adam_opts
extern "C" int mmda_clamp_adam_opts(float* p, const float* acc, const float* g, float* m, float* v, int64_t n, const mmda_run* runs,
                                    int n_runs, int64_t items, float lr, float clip, float grad_scale, int step,
                                    const mmda_adam_opts* opts, void* stream) {
  if (!adam_opts_ok(opts) || ((uintptr_t)opts->scale_dev & 3)) return MMDA_EINVAL;
  const AdamHyper h = adam_hyper(lr, clip, grad_scale, step, *opts);
  if (!runs && n_runs == 0 && items == 0) return mmda_adam_launch(p, acc, g, m, v, n, nullptr, h, kNoWait, stream);
  const RunTable t{runs, n_runs, items};
  return mmda_adam_launch(p, acc, g, m, v, 0, &t, h, kNoWait, stream);
}

// ---- gradient norm and scale: host side
namespace {
int norm_blocks(int64_t n, const RunTable* table) { return stream_blocks(table ? table->items : n / 4); }
}  // namespace

extern "C" int64_t mmda_grad_norm_partials(int64_t n_or_items) {
  if (n_or_items < 0) return MMDA_EINVAL;
  if (n_or_items >= (int64_t)2048 * 256) return 2048;      // (the grid's cap)
  return stream_blocks(n_or_items);                        // >= the blocks of a dense launch over n floats and of a run launch over n items
}

// internal.h: the two launches behind mmda_grad_norm (and misa_step.hip's)
int mmda_grad_norm_launch(const float* g, const float* acc, int64_t n, const RunTable* table, float max_norm, float grad_scale,
                          double* partials, int64_t partials_capacity, float* out2, void* stream) {
  if (!g || !partials || !out2 || !(max_norm >= 0.f)) return MMDA_EINVAL;
  if (table ? (table->n_runs < 0 || table->items < 0) : n < 0) return MMDA_EINVAL;
  if (((uintptr_t)g | (uintptr_t)acc) & 15 || ((uintptr_t)partials & 7) || ((uintptr_t)out2 & 3)) return MMDA_EINVAL;
  const bool empty = table ? (table->n_runs == 0 || table->items == 0) : n == 0;
  if (table && !empty && !table->runs) return MMDA_EINVAL;
  const int nb = empty ? 0 : norm_blocks(n, table);
  if (nb > partials_capacity) return MMDA_EINVAL;
  if (nb > 0) {
    const mmda_run* runs = table ? table->runs : nullptr;
    const int n_runs = table ? table->n_runs : 0;
    const int64_t items = table ? table->items : 0;
    if (acc) hipLaunchKernelGGL(grad_norm_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)stream, acc, g, n, runs, n_runs, items, partials);
    else hipLaunchKernelGGL(grad_norm_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)stream, acc, g, n, runs, n_runs, items, partials);
    MMDA_CHECK_LAUNCH("mmda_grad_norm");
  }
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, nb, grad_scale, max_norm, out2);
  MMDA_CHECK_LAUNCH("mmda_grad_norm/finish");
  return MMDA_OK;
}

extern "C" int mmda_grad_norm(const float* g, const float* acc, int64_t n, const mmda_run* runs, int n_runs, int64_t items, float max_norm,
                              float grad_scale, double* partials, int64_t partials_capacity, float* out2, void* stream) {
  if (!runs && n_runs == 0 && items == 0)
    return mmda_grad_norm_launch(g, acc, n, nullptr, max_norm, grad_scale, partials, partials_capacity, out2, stream);
  const RunTable t{runs, n_runs, items};
  return mmda_grad_norm_launch(g, acc, 0, &t, max_norm, grad_scale, partials, partials_capacity, out2, stream);
}

extern "C" int mmda_grad_scale(float* g, int64_t n, const mmda_run* runs, int n_runs, int64_t items, const float* scale_dev, void* stream) {
  if (!g || !scale_dev || n < 0 || n_runs < 0 || items < 0 || ((uintptr_t)g & 15) || ((uintptr_t)scale_dev & 3)) return MMDA_EINVAL;
  const bool table = runs || n_runs != 0 || items != 0;
  if (table ? (n_runs == 0 || items == 0) : n == 0) return MMDA_OK;
  if (table && !runs) return MMDA_EINVAL;
  const Scale f{g, scale_dev};
  return table ? launch_runs("mmda_grad_scale", RunTable{runs, n_runs, items}, f, kNoWait, stream)
               : launch_stream("mmda_grad_scale", n, f, kNoWait, stream);
}

extern "C" int mmda_clamp_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                               float eps, float clip, float grad_scale, int step, void* stream) {
  return mmda_adam_launch(p, nullptr, g, m, v, n, nullptr, AdamHyper{lr, beta1, beta2, eps, clip, grad_scale, step}, kNoWait, stream);
}

// acc == nullptr (one micro-batch: no sum): mmda_clamp_adam
extern "C" int mmda_clamp_adam_sum(float* p, const float* acc, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                                   float beta2, float eps, float clip, float grad_scale, int step, void* stream) {
  return mmda_adam_launch(p, acc, g, m, v, n, nullptr, AdamHyper{lr, beta1, beta2, eps, clip, grad_scale, step}, kNoWait, stream);
}

extern "C" int mmda_grad_accumulate(float* acc, const float* g, int64_t n, int first, void* stream) {
  if (!acc || !g || n < 0) return MMDA_EINVAL;
  if (((uintptr_t)acc | (uintptr_t)g) & 15) return MMDA_EINVAL;                                // float4 path
  if (n == 0) return MMDA_OK;
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, acc, g, n, first ? 1 : 0);
  MMDA_CHECK_LAUNCH("mmda_grad_accumulate");
  return MMDA_OK;
}

// ---- trainable runs (frozen parameters): host side
// internal (misa.hip): mmda_runs_build that never merges two ranges across one of `cuts` (bucket offsets, multiples of 4, inside no
// range), so that the runs of the bucket between two cuts are a slice of the table
int64_t mmda_runs_build_cut(const int64_t* begin, const int64_t* len, int n, int64_t bucket_floats, const int64_t* cuts, int n_cuts,
                            mmda_run* out, int* n_out) {
  if (n < 0 || bucket_floats < 0 || !n_out || (n > 0 && (!begin || !len || !out)) || (n_cuts > 0 && !cuts)) return MMDA_EINVAL;
  int k = 0;
  int64_t end = 0, items = 0;                            // where the last range ended; work items so far
  for (int i = 0; i < n; ++i) {
    if (len[i] < 0 || begin[i] < end || begin[i] > bucket_floats || len[i] > bucket_floats - begin[i]) return MMDA_EINVAL;
    if (len[i] == 0) continue;
    bool at_cut = false;
    for (int c = 0; c < n_cuts; ++c) at_cut = at_cut || cuts[c] == begin[i];
    if (k > 0 && begin[i] == end && !at_cut) {
      mmda_run& r = out[k - 1];
      items -= ((r.begin + r.len - 1) >> 2) - (r.begin >> 2) + 1;
      r.len += len[i];
      items += ((r.begin + r.len - 1) >> 2) - (r.begin >> 2) + 1;
    } else {
      out[k++] = mmda_run{begin[i], len[i], items};
      items += ((begin[i] + len[i] - 1) >> 2) - (begin[i] >> 2) + 1;
    }
    end = begin[i] + len[i];
  }
  *n_out = k;
  return items;
}

extern "C" int64_t mmda_runs_build(const int64_t* begin, const int64_t* len, int n, int64_t bucket_floats, mmda_run* out, int* n_out) {
  return mmda_runs_build_cut(begin, len, n, bucket_floats, nullptr, 0, out, n_out);
}

extern "C" int mmda_clamp_adam_runs(float* p, const float* g, float* m, float* v, const mmda_run* runs, int n_runs, int64_t items, float lr,
                                    float beta1, float beta2, float eps, float clip, float grad_scale, int step, void* stream) {
  const RunTable t{runs, n_runs, items};
  return mmda_adam_launch(p, nullptr, g, m, v, 0, &t, AdamHyper{lr, beta1, beta2, eps, clip, grad_scale, step}, kNoWait, stream);
}

// acc == nullptr: mmda_clamp_adam_runs
extern "C" int mmda_clamp_adam_sum_runs(float* p, const float* acc, const float* g, float* m, float* v, const mmda_run* runs, int n_runs,
                                        int64_t items, float lr, float beta1, float beta2, float eps, float clip, float grad_scale, int step,
                                        void* stream) {
  const RunTable t{runs, n_runs, items};
  return mmda_adam_launch(p, acc, g, m, v, 0, &t, AdamHyper{lr, beta1, beta2, eps, clip, grad_scale, step}, kNoWait, stream);
}

extern "C" int mmda_clamp_rmsprop_runs(float* p, const float* g, float* square_avg, const mmda_run* runs, int n_runs, int64_t items,
                                       float lr, float alpha, float eps, float clip, float grad_scale, void* stream) {
  if (!p || !g || !square_avg || n_runs < 0 || items < 0) return MMDA_EINVAL;
  if (n_runs == 0 || items == 0) return MMDA_OK;
  if (!runs) return MMDA_EINVAL;
  const RunRmsprop f{p, g, square_avg, lr, alpha, eps, clip, grad_scale};
  return launch_runs("mmda_clamp_rmsprop_runs", RunTable{runs, n_runs, items}, f, kNoWait, stream);
}

// internal (misa_forward.hip): a[0 .. na) = b[0 .. nb) = 0 in ONE launch (two memsets are two launches of ~5 us each on a latency-bound chain)
int mmda_zero2(float* a, int64_t na, float* b, int64_t nb, void* stream) {
  if (na < 0 || nb < 0 || (na && !a) || (nb && !b)) return MMDA_EINVAL;
  if (((uintptr_t)a | (uintptr_t)b) & 15 || (na & 3) || (nb & 3)) {           // odd shapes: the runtime's fills
    if (na && hipMemsetAsync(a, 0, sizeof(float) * na, (hipStream_t)stream) != hipSuccess) return MMDA_ELAUNCH;
    if (nb && hipMemsetAsync(b, 0, sizeof(float) * nb, (hipStream_t)stream) != hipSuccess) return MMDA_ELAUNCH;
    return MMDA_OK;
  }
  const int64_t n4 = (na + nb) >> 2;
  if (n4 == 0) return MMDA_OK;
  hipLaunchKernelGGL(zero2_kernel, dim3(stream_blocks(n4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<float4*>(a), na >> 2,
                     reinterpret_cast<float4*>(b), nb >> 2);
  MMDA_CHECK_LAUNCH("mmda_zero2");
  return MMDA_OK;
}

extern "C" int mmda_mark_rows(unsigned char* mask, int rows, const int64_t* ids, int n, void* stream) {
  if (!mask || !ids || rows <= 0 || n < 0) return MMDA_EINVAL;
  if (hipMemsetAsync(mask, 0, (size_t)rows, (hipStream_t)stream) != hipSuccess) return MMDA_ELAUNCH;
  if (n == 0) return MMDA_OK;
  hipLaunchKernelGGL(mark_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, mask, rows, ids, n);
  MMDA_CHECK_LAUNCH("mmda_mark_rows");
  return MMDA_OK;
}

extern "C" int mmda_clamp_adam_rows(float* p, const float* g, float* m, float* v, int rows, int dim, const unsigned char* mask, int want,
                                    float lr, float beta1, float beta2, float eps, float clip, float grad_scale, int step, void* stream) {
  if (!p || !g || !m || !v || !mask || rows < 0 || dim <= 0 || step < 1) return MMDA_EINVAL;
  if (rows == 0) return MMDA_OK;
  const Adam<false> f{adam_args(p, nullptr, g, m, v, AdamHyper{lr, beta1, beta2, eps, clip, grad_scale, step})};
  const int vec = (dim & 3) == 0 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  int blocks = (rows + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(rows_kernel<Adam<false>>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rows, dim, mask, want, vec, f);
  MMDA_CHECK_LAUNCH("mmda_clamp_adam_rows");
  return MMDA_OK;
}

extern "C" int mmda_clamp_adam_rows_opts(float* p, const float* g, float* m, float* v, int rows, int dim, const unsigned char* mask, int want,
                                         float lr, float clip, float grad_scale, int step, const mmda_adam_opts* opts, void* stream) {
  if (!adam_opts_ok(opts) || ((uintptr_t)opts->scale_dev & 3)) return MMDA_EINVAL;
  if (!p || !g || !m || !v || !mask || rows < 0 || dim <= 0 || step < 1) return MMDA_EINVAL;
  if (rows == 0) return MMDA_OK;
  const AdamHyper h = adam_hyper(lr, clip, grad_scale, step, *opts);
  const int vec = (dim & 3) == 0 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  int blocks = (rows + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  const AdamArgs a = adam_args(p, nullptr, g, m, v, h);
  if (adam_plain(h)) {
    hipLaunchKernelGGL(rows_kernel<Adam<false>>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rows, dim, mask, want, vec, Adam<false>{a});
  } else {
    const AdamOpt<false> f{adam_opt_args(a, h)};
    hipLaunchKernelGGL(rows_kernel<AdamOpt<false>>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rows, dim, mask, want, vec, f);
  }
  MMDA_CHECK_LAUNCH("mmda_clamp_adam_rows_opts");
  return MMDA_OK;
}

extern "C" int mmda_clamp(float* g, int64_t n, float clip, void* stream) {
  if (!g || n < 0) return MMDA_EINVAL;
  if (n == 0) return MMDA_OK;
  hipLaunchKernelGGL(clamp_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, g, n, clip);
  MMDA_CHECK_LAUNCH("mmda_clamp");
  return MMDA_OK;
}

extern "C" int mmda_clamp_rmsprop(float* p, const float* g, float* square_avg, int64_t n, float lr, float alpha, float eps, float clip,
                                  float grad_scale, void* stream) {
  if (!p || !g || !square_avg || n < 0) return MMDA_EINVAL;
  if (n == 0) return MMDA_OK;
  hipLaunchKernelGGL(clamp_rmsprop_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, square_avg, n, lr, alpha, eps,
                     clip, grad_scale);
  MMDA_CHECK_LAUNCH("mmda_clamp_rmsprop");
  return MMDA_OK;
}
