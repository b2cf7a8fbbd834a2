// Modality masking (mmda_amd/modality.py): a batch with some of its three inputs -- 0 = text, 1 = visual, 2 = acoustic --
// blanked, and what each input contributes to a value.  A keep set is three bits, bit m set = modality m is kept.  Blanking a column:
// every word id at t < len becomes unk_id (padding keeps pad_id), the column's visual / acoustic rows become 0.0f; lengths and labels
// are left alone and nothing is rescaled.  Three launches: the masked form of collate_gather_kernel, the out-of-place mask of a batch
// that is already made, and the Shapley collector over the eight keep sets' values.
#include "internal.h"

namespace {

enum { SITE_MODALITY = 11 };                                   // the next id after misa_handle.h's dropout sites

using DropP = mmda_modality_p;

// The random keep set of SAMPLE s (a dataset index, not a batch position): modality m is dropped iff p_m > 0 && u_m < p_m, the fp32
// compare of drop_mul, u_m from rng_u32(seed, SITE_MODALITY, 3 s + m); a draw that drops all three drops none.
__device__ __forceinline__ int random_keep(uint64_t seed, const DropP& p, int64_t s) {
  int drop = 0;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    if (p.p[m] > 0.0f) {
      const float u = (float)(rng_u32(seed, SITE_MODALITY, (uint64_t)(3 * s + m)) >> 8) * (1.0f / 16777216.0f);
      if (u < p.p[m]) drop |= 1 << m;
    }
  }
  return drop == 7 ? 7 : 7 & ~drop;
}

// One time position of one column, the three sources it READS as template arguments: every instantiation issues its loads (of the kept
// modalities only) with no branch between them and its stores (0.19 us per launch at B = 256 against an if / else per modality).
// `fill` is the id of a position whose word is not read: pad_id past the sample's length, unk_id inside it.
template <bool RT, bool RV, bool RA>
__device__ __forceinline__ void put_position(const int32_t* __restrict__ words, const float* __restrict__ visual,
                                             const float* __restrict__ acoustic, int64_t src, int64_t dst, int dv, int da, int lane,
                                             int64_t fill, int64_t* __restrict__ out_ids, float* __restrict__ out_v,
                                             float* __restrict__ out_a) {
  for (int c = lane; c < dv; c += 64) out_v[dst * dv + c] = RV ? visual[src * dv + c] : 0.f;
  for (int c = lane; c < da; c += 64) out_a[dst * da + c] = RA ? acoustic[src * da + c] : 0.f;
  if (lane == 0) out_ids[dst] = RT ? (int64_t)words[src] : fill;
}

// collate_gather_kernel's grid and wave-per-column layout (collate.hip) with the column's keep set computed once per wave next to
// order[b]; the keep set is wave-uniform, so every branch below is.  A dropped modality is written without its source being read.
// SCALAR_B: the wave's column index is read through readfirstlane, so b, the sample index, its offsets and its keep set are scalars
// (scalar loads, the three hashes on the scalar unit).  Measured: that form is the faster one while the launch is a
// few hundred workgroups whose time is the chain of dependent loads (B = 32: 2.9 against 3.2 us), and the slower one once the grid
// fills the device (B = 256, 2048 workgroups: 5.3 against 4.7 us), so the launcher picks by the grid's size.
template <bool SCALAR_B>
__global__ __launch_bounds__(256) void collate_gather_masked_kernel(const int32_t* __restrict__ words, const float* __restrict__ visual,
                                                                    const float* __restrict__ acoustic,
                                                                    const int64_t* __restrict__ offsets, const float* __restrict__ emo,
                                                                    const float* __restrict__ sentiment,
                                                                    const int32_t* __restrict__ order, int B, int T, int dv, int da,
                                                                    int pad_id, int keep_const, DropP p, int any_p, uint64_t seed,
                                                                    int unk_id, int64_t* __restrict__ out_ids, float* __restrict__ out_v,
                                                                    float* __restrict__ out_a, float* __restrict__ out_emo,
                                                                    float* __restrict__ out_y, uint8_t* __restrict__ out_keep) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)(threadIdx.x >> 6);
  const int b = (int)blockIdx.x * 4 + (SCALAR_B ? __builtin_amdgcn_readfirstlane(wave) : wave);
  if (b >= B) return;                                        // wave-uniform
  const int64_t s = order[b];
  const int64_t o0 = offsets[s];
  const int64_t len = offsets[s + 1] - o0;
  const int keep = (any_p ? random_keep(seed, p, s) : 7) & keep_const;
  if (blockIdx.y == 0) {                                     // the labels and the keep set of the column, once
    if (out_emo && lane < 6) out_emo[(int64_t)b * 6 + lane] = emo[s * 6 + lane];
    if (lane == 6) out_y[b] = sentiment[s];
    if (out_keep && lane == 7) out_keep[b] = (uint8_t)keep;
  }
  for (int t = (int)blockIdx.y; t < T; t += (int)gridDim.y) {
    const int64_t dst = (int64_t)t * B + b;
    const int64_t src = o0 + t;
    const int reads = t < len ? keep : 0;                    // bit m: modality m of this position is copied from the dataset
    const int64_t fill = t < len ? (int64_t)unk_id : (int64_t)pad_id;
#define MMDA_PUT(RT, RV, RA) put_position<RT, RV, RA>(words, visual, acoustic, src, dst, dv, da, lane, fill, out_ids, out_v, out_a)
    switch (reads) {
      case 7: MMDA_PUT(true, true, true); break;
      case 6: MMDA_PUT(false, true, true); break;
      case 5: MMDA_PUT(true, false, true); break;
      case 4: MMDA_PUT(false, false, true); break;
      case 3: MMDA_PUT(true, true, false); break;
      case 2: MMDA_PUT(false, true, false); break;
      case 1: MMDA_PUT(true, false, false); break;
      default: MMDA_PUT(false, false, false); break;
    }
#undef MMDA_PUT
  }
}

// The same grid over a batch that exists already: ids (T, B), v (T, B, dv), a (T, B, da) -> masked copies.  The keep set of column b
// is keep[b] (& 7), or keep_const when keep is NULL.  Padding is recognised by the id alone (pad_id is reserved: never a word), so no
// lengths are read; the padding rows of v / a are zero already and are copied like any other row.  The inputs are only read.
template <bool KV, bool KA>
__device__ __forceinline__ void mask_position(const int64_t* __restrict__ ids, const float* __restrict__ v, const float* __restrict__ a,
                                              int64_t r, int dv, int da, int lane, bool kt, int64_t pad_id, int64_t unk_id,
                                              int64_t* __restrict__ out_ids, float* __restrict__ out_v, float* __restrict__ out_a) {
  for (int c = lane; c < dv; c += 64) out_v[r * dv + c] = KV ? v[r * dv + c] : 0.f;
  for (int c = lane; c < da; c += 64) out_a[r * da + c] = KA ? a[r * da + c] : 0.f;
  if (lane == 0) {
    const int64_t id = ids[r];
    out_ids[r] = (kt || id == pad_id) ? id : unk_id;
  }
}

__global__ __launch_bounds__(256) void modality_mask_kernel(const int64_t* __restrict__ ids, const float* __restrict__ v,
                                                            const float* __restrict__ a, int T, int B, int dv, int da,
                                                            const uint8_t* __restrict__ keep_col, int keep_const, int pad_id, int unk_id,
                                                            int64_t* __restrict__ out_ids, float* __restrict__ out_v,
                                                            float* __restrict__ out_a) {
  const int lane = threadIdx.x & 63;
  const int b = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;                                        // wave-uniform
  const int keep = keep_col ? (int)keep_col[b] & 7 : keep_const;
  const bool kt = keep & 1;
  for (int t = (int)blockIdx.y; t < T; t += (int)gridDim.y) {
    const int64_t r = (int64_t)t * B + b;
#define MMDA_MASK(KV, KA) mask_position<KV, KA>(ids, v, a, r, dv, da, lane, kt, pad_id, unk_id, out_ids, out_v, out_a)
    switch (keep >> 1) {
      case 3: MMDA_MASK(true, true); break;
      case 2: MMDA_MASK(false, true); break;
      case 1: MMDA_MASK(true, false); break;
      default: MMDA_MASK(false, false); break;
    }
#undef MMDA_MASK
  }
}

// Exact Shapley values of three players.  One thread per (row i, class c), e = i C + c: it reads V[k][e], k = 0 .. 7, once (consecutive
// threads on consecutive floats in each of the eight planes) and writes
//   phi[i][m][c] = sum over the four S without m, in ascending S, of w(|S|) (V[S | m] - V[S]), w(0) = w(2) = 1/3, w(1) = 1/6;
//   loo[i][m][c] = V[7] - V[7 ^ m];
//   dominant[i][c] = the lowest m among the non-NaN phi_m that attain their maximum (strict > in ascending m), -1 when all are NaN.
// counts[m][c] = rows that m dominates: the workgroup's threads add into 3 C LDS integers when C <= ATTRIB_LDS_C (a workgroup of 256
// consecutive e touches every class about 256 / C times), and one 64-bit integer add per non-zero cell goes out; wider C adds straight
// to memory.  Integer sums: the same bits on every run.
constexpr int ATTRIB_LDS_C = 256;

__global__ __launch_bounds__(256) void modality_attrib_kernel(const float* __restrict__ V, int64_t nC, int C, float* __restrict__ phi,
                                                              float* __restrict__ loo, int32_t* __restrict__ dominant,
                                                              unsigned long long* __restrict__ counts) {
  __shared__ int cnt[3 * ATTRIB_LDS_C];
  const bool lds = C <= ATTRIB_LDS_C;
  if (lds) {
    for (int k = threadIdx.x; k < 3 * C; k += 256) cnt[k] = 0;
    __syncthreads();
  }
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < nC) {
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = V[(int64_t)k * nC + e];
    const int64_t i = e / C;
    const int c = (int)(e - i * C);
    const float w3 = 1.0f / 3.0f, w6 = 1.0f / 6.0f;
    float best = 0.f;
    int dom = -1;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int bit = 1 << m;
      const int s1 = m == 0 ? 2 : 1, s2 = m == 2 ? 2 : 4;    // the two one-element sets without m, ascending
      float f = w3 * (x[bit] - x[0]);
      f += w6 * (x[s1 | bit] - x[s1]);
      f += w6 * (x[s2 | bit] - x[s2]);
      f += w3 * (x[7] - x[7 ^ bit]);
      const int64_t o = (i * 3 + m) * C + c;
      phi[o] = f;
      loo[o] = x[7] - x[7 ^ bit];
      if (f == f && (dom < 0 || f > best)) { best = f; dom = m; }
    }
    dominant[e] = dom;
    if (dom >= 0) {
      if (lds) atomicAdd(&cnt[dom * C + c], 1);
      else atomicAdd(&counts[(int64_t)dom * C + c], 1ull);
    }
  }
  if (lds) {
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * C; k += 256)
      if (cnt[k]) atomicAdd(&counts[k], (unsigned long long)cnt[k]);
  }
}

// the scalar-column form of the masked gather up to this many workgroups (measured at 400 and at 2048; the crossover in between is not)
constexpr int64_t MASKED_SCALAR_MAX_WGS = 512;

inline bool bad_p(float p) { return !(p >= 0.0f && p < 1.0f); }      // NaN included

inline dim3 column_grid(int B, int T) {                     // mmda_collate_gather's
  const int bx = ceil_div(B, 4);
  int by = 2048 / bx;
  if (by < 1) by = 1;
  if (by > T) by = T;
  return dim3(bx, by);
}

}  // namespace

extern "C" int mmda_collate_gather_masked(const int32_t* words, const float* visual, const float* acoustic, const int64_t* offsets,
                                          const float* emo, const float* sentiment, const int32_t* order, int B, int T, int dv, int da,
                                          int pad_id, int keep_const, mmda_modality_p p, uint64_t seed, int unk_id, int64_t* out_ids,
                                          float* out_v, float* out_a, float* out_emo, float* out_y, uint8_t* out_keep, void* stream) {
  if (!words || !visual || !acoustic || !offsets || !sentiment || !order || !out_ids || !out_v || !out_a || !out_y) return MMDA_EINVAL;
  if (B <= 0 || T <= 0 || dv <= 0 || da <= 0) return MMDA_EINVAL;
  if (!emo && out_emo) return MMDA_EINVAL;
  if (keep_const < 0 || keep_const > 7) return MMDA_EINVAL;
  if (bad_p(p.p[0]) || bad_p(p.p[1]) || bad_p(p.p[2])) return MMDA_EINVAL;

  const int any_p = p.p[0] > 0.0f || p.p[1] > 0.0f || p.p[2] > 0.0f;
  const dim3 grid = column_grid(B, T);
  if ((int64_t)grid.x * grid.y <= MASKED_SCALAR_MAX_WGS)
    hipLaunchKernelGGL(collate_gather_masked_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, words, visual, acoustic, offsets, emo,
                       sentiment, order, B, T, dv, da, pad_id, keep_const, p, any_p, seed, unk_id, out_ids, out_v, out_a, out_emo, out_y,
                       out_keep);
  else
    hipLaunchKernelGGL(collate_gather_masked_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, words, visual, acoustic, offsets, emo,
                       sentiment, order, B, T, dv, da, pad_id, keep_const, p, any_p, seed, unk_id, out_ids, out_v, out_a, out_emo, out_y,
                       out_keep);
  MMDA_CHECK_LAUNCH("mmda_collate_gather_masked");
  return MMDA_OK;
}

extern "C" int mmda_modality_mask(const int64_t* ids, const float* v, const float* a, int T, int B, int dv, int da, const uint8_t* keep,
                                  int keep_const, int pad_id, int unk_id, int64_t* out_ids, float* out_v, float* out_a, void* stream) {
  if (!ids || !v || !a || !out_ids || !out_v || !out_a) return MMDA_EINVAL;
  if (B <= 0 || T <= 0 || dv <= 0 || da <= 0) return MMDA_EINVAL;
  if (keep_const < 0 || keep_const > 7) return MMDA_EINVAL;
  if ((const void*)ids == (const void*)out_ids || v == out_v || a == out_a) return MMDA_EINVAL;      // out of place only
  hipLaunchKernelGGL(modality_mask_kernel, column_grid(B, T), dim3(256), 0, (hipStream_t)stream, ids, v, a, T, B, dv, da, keep,
                     keep_const, pad_id, unk_id, out_ids, out_v, out_a);
  MMDA_CHECK_LAUNCH("mmda_modality_mask");
  return MMDA_OK;
}

extern "C" int mmda_modality_attrib(const float* V, int64_t n, int C, float* phi, float* loo, int32_t* dominant, int64_t* counts,
                                    void* stream) {
  if (!V || !phi || !loo || !dominant || !counts) return MMDA_EINVAL;
  if (n <= 0 || C <= 0) return MMDA_EINVAL;
  const int64_t nC = n * (int64_t)C;
  const int64_t blocks = ceil_div64(nC, 256);
  if (blocks > 0x7fffffff) return MMDA_EINVAL;
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 3 * (size_t)C, (hipStream_t)stream) != hipSuccess) return MMDA_ELAUNCH;
  hipLaunchKernelGGL(modality_attrib_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, V, nC, C, phi, loo, dominant,
                     reinterpret_cast<unsigned long long*>(counts));
  MMDA_CHECK_LAUNCH("mmda_modality_attrib");
  return MMDA_OK;
}
