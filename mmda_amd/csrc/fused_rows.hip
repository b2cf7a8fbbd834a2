// The row-local stretches of the fusion block's backward pass, one launch each (see fused_rows.h).
// Workgroup = 512 threads = 8 waves, rows of `nb` samples (1 by default: the MFMA tile is then 6 of 16 rows full, but what a stage waits
// for is its weights, and twice the workgroups halve the LayerNorm / attention rounds; 2 = twelve token rows per tile).  GEMM stages use
// v_mfma_f32_16x16x4_f32 (exact f32; hs = 128: every product is a whole number of 128-deep rounds) with operands global -> registers -> MFMA as in gemm_skinny.hip: wave w owns output columns
// 16 w .. 16 w + 15 (hs = 128 = 8 waves x 16), walks the whole reduction itself, and applies its epilogue straight from the accumulators.
// The six problems of d_x6 and the three of d_orig each become ONE accumulator chain per wave: the products that differ per modality
// run over the same 16-row tile with the rows of the other modalities zeroed.
#include "common.h"
#include "internal.h"
#include "rowlocal.h"
#include "fused_rows.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f4;
constexpr int FR_THREADS = 512;

// acc += A_row(lane & 15)[0..K) . Bt_row(lane & 15)[0..K)^T for the 16 x 16 tile (rows: the lanes' A rows, columns: the lanes' Bt rows).
// arow == nullptr: a zero row.  K % 16 == 0, rows 16-byte aligned.  Rounds of eight 16-deep chunks; the loads of round r + 1 are issued
// before the MFMAs of round r (two register sets: a stage is a chain of memory latencies, the MFMAs hide behind the next one).
struct MacRound { f4 a[8], b[8]; };
// One round = 128 of the reduction for a 16 x 16 tile: A rows from the workgroup's LDS image (stage_rows), the wave's 16 weight rows
// from global THROUGH a wave-private LDS block.  Read straight into the fragment layout, the 16 rows of a wave are sixteen 64-byte
// requests per load instruction, and the rate at which a CU's memory pipeline takes requests (not bytes) is what paces a stage; read as
// the lines lie -- lane l takes 16 bytes at offset 16 l of two whole 512-byte row segments per instruction -- they are eight 128-byte
// requests, and the fragments come out of LDS (rows 132 floats apart: the sixteen rows of a b128 read on distinct banks).
constexpr int WL_LD = 128 + 4;
struct WRows { f4 g[8]; };
// issue the loads of one round: `bblk` = first of the wave's 16 weight rows at the round's k, `ldb` = floats between rows
__device__ __forceinline__ void wrows_load(WRows& W, const float* __restrict__ bblk, int ldb, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) W.g[j] = *reinterpret_cast<const f4*>(bblk + (int64_t)(2 * j + (lane >> 5)) * ldb + 4 * (lane & 31));
}
__device__ __forceinline__ void wrows_to_lds(const WRows& W, float* wl, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<f4*>(wl + (2 * j + (lane >> 5)) * WL_LD + 4 * (lane & 31)) = W.g[j];
}
// a lane's float4 at k = 16 c + 4 (lane >> 4) of its row feeds component s to the (c, s)-th MFMA (a permutation of k that A and B share)
__device__ __forceinline__ void mac_frags(MacRound& R, const float* arow /* LDS or nullptr = zero row */, const float* wl, int lane) {
  const int r16 = lane & 15, g = lane >> 4;
  const f4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    R.a[c] = arow ? *reinterpret_cast<const f4*>(arow + 16 * c + 4 * g) : z;
    R.b[c] = *reinterpret_cast<const f4*>(wl + r16 * WL_LD + 16 * c + 4 * g);
  }
}
__device__ __forceinline__ void mac_run(f32x4& acc, const MacRound& R) {
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(R.a[c][s], R.b[c][s], acc, 0, 0, 0);
}
// NR rounds into one accumulator; round r multiplies A row ar[r] (LDS; nullptr = zeros) with the wave's 16 weight rows at bblk[r] (row
// stride ldb[r]).  The global loads of round r + 1 are in flight while round r's fragments are read and multiplied.
template <int NR>
__device__ __forceinline__ void tile_mac_chain(f32x4& acc, const float* const (&ar)[NR], const float* const (&bblk)[NR], const int (&ldb)[NR],
                                               int lane, float* wl /* this wave's 16 x WL_LD floats of LDS */) {
  WRows W;
  MacRound R;
  wrows_load(W, bblk[0], ldb[0], lane);
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    wrows_to_lds(W, wl, lane);                           // (the previous round's fragment reads are in registers: program order in LDS)
    if (r + 1 < NR) wrows_load(W, bblk[r + 1], ldb[r + 1], lane);
    mac_frags(R, ar[r], wl, lane);
    mac_run(acc, R);
  }
}

// sum of n values `stride` floats apart, added in index order; sixteen loads in flight at a time (one at a time is n memory latencies)
__device__ __forceinline__ float sum_parts(const float* __restrict__ p, int n, int64_t stride) {
  float acc = 0.f;
  int q = 0;
  for (; q + 16 <= n; q += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p[(q + u) * stride];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc += v[u];
  }
  for (; q < n; ++q) acc += p[q * stride];
  return acc;
}

// The same sums for whole rows, workgroup-wide: `groups` = 16-byte column groups (row_off(g) = the group's float offset inside a
// partial); the partials in two halves, each half by a thread of its own (sixteen 16-byte loads in flight: 64 partials are two batches
// of latency per thread instead of four 4-byte batches), the two half sums -- in slice order each -- meet in LDS and
// finish(g, lower half + upper half) stores them.  lds: 2 * groups float4.  Ends with a workgroup barrier.
template <typename RowOff, typename Finish>
__device__ __forceinline__ void sum_parts_rows(const float* __restrict__ parts, int n, int64_t stride, int groups, RowOff row_off, f4* lds,
                                               Finish finish) {
  const int n0 = (n + 1) >> 1;
  for (int it = threadIdx.x; it < 2 * groups; it += FR_THREADS) {
    const int gi = it % groups, half = it / groups;
    const float* p = parts + row_off(gi) + (int64_t)(half ? n0 : 0) * stride;
    const int cnt = half ? n - n0 : n0;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    int q = 0;
    for (; q + 16 <= cnt; q += 16) {
      f4 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = *reinterpret_cast<const f4*>(p + (q + u) * stride);
#pragma unroll
      for (int u = 0; u < 16; ++u) acc += v[u];
    }
    for (; q < cnt; ++q) acc += *reinterpret_cast<const f4*>(p + q * stride);
    lds[half * groups + gi] = acc;
  }
  __syncthreads();
  for (int gi = threadIdx.x; gi < groups; gi += FR_THREADS) finish(gi, lds[gi] + lds[groups + gi]);
  __syncthreads();
}

// stage boundary: this workgroup's global stores are visible to all of its waves
__device__ __forceinline__ void stage_sync() {
  __threadfence_block();
  __syncthreads();
}

// LDS image of a stage's A rows: row r at lds + r * (K + 4) floats (the + 4 puts the sixteen rows a b128 read touches on distinct banks).
// src_of(r): the global row (K floats, 16-byte aligned) or nullptr for a zero row.  Ends with a workgroup barrier.
constexpr int LDS_A_FLOATS = 12 * (384 + 4) + 18 * (128 + 4);      // the largest stage: twelve d_qkv rows + their d_recon rows
template <typename SrcOf>
__device__ __forceinline__ void stage_rows(float* lds, int nrows, int K, SrcOf src_of) {
  const int per_row = K >> 2;
  for (int e = threadIdx.x; e < nrows * per_row; e += FR_THREADS) {
    const int r = e / per_row, c = e % per_row;
    const float* src = src_of(r);
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f4*>(lds + r * (K + 4) + 4 * c) = src ? *reinterpret_cast<const f4*>(src + 4 * c) : z;
  }
  __syncthreads();
}

// LayerNorm backward of the rows `row_of(i)`, i < nrows, waves round robin; dgamma / dbeta of the workgroup's rows summed over its
// waves in LDS (fixed order) and left as ONE partial row each in `part` (2 x 128 floats: gamma, beta) -- mmda_fused_pg_finish adds the
// partials of all workgroups in order.  n <= 128.
template <typename RowOf>
__device__ __forceinline__ void ln_bwd_rows(const mmda_ln_bwd_args& a, int nrows, RowOf row_of, float* red /* 2 x 8 x 128 floats */,
                                            float* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dg[2] = {0.f, 0.f}, db[2] = {0.f, 0.f};
  for (int i = wave; i < nrows; i += FR_THREADS / 64) ln_bwd_row<2>(a, row_of(i), lane, dg, db);
  if (part == nullptr) return;                                        // workgroup-uniform
#pragma unroll
  for (int q = 0; q < 2; ++q) { red[(0 * 8 + wave) * 128 + q * 64 + lane] = dg[q]; red[(1 * 8 + wave) * 128 + q * 64 + lane] = db[q]; }
  __syncthreads();
  for (int i = threadIdx.x; i < 128; i += FR_THREADS) {
    float gsum = 0.f, bsum = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) { gsum += red[(0 * 8 + w) * 128 + i]; bsum += red[(1 * 8 + w) * 128 + i]; }
    part[i] = i < a.n ? gsum : 0.f;
    part[128 + i] = i < a.n ? bsum : 0.f;
  }
  __syncthreads();                                                   // `red` is free again
}
// slot k of sample b in pg_parts (B, 5, 2, 128)
__device__ __forceinline__ float* pg_slot(float* parts, int b, int k) { return parts ? parts + ((int64_t)b * FUSED_PG_SLOTS + k) * 256 : nullptr; }
// the workgroup-wide sums live in the slot of the workgroup's FIRST sample: the slots of its other samples are zero
__device__ __forceinline__ void pg_zero_rest(float* parts, int b0, int nb, int k) {
  if (!parts) return;
  for (int e = threadIdx.x; e < (nb - 1) * 256; e += FR_THREADS) pg_slot(parts, b0 + 1 + e / 256, k)[e % 256] = 0.f;
}

// rec_part[i] = d_recon[i] W_rec[i] for the modality rows of `nb` samples (the term fused_bwd_a_kernel adds into d_x6 of the private and
// the shared token of modality i): its operands exist before the backward pass starts, so workgroups [nblk, 2 nblk) of the stretch-C
// launch make it beside that stretch instead of three extra rounds in the middle of stretch A's chain
__device__ __forceinline__ void rec_part_rows(const FusedBwdC& P, int b0, int nb, float* lds_a, float* lds_w) {
  const int B = P.B, hs = P.hs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int nmod = 3 * nb;
  const bool mok = r16 < nmod;
  const int mi = mok ? r16 / nb : 0;
  const int col = wave * 16 + r16;
  stage_rows(lds_a, nmod, hs, [&](int r) { return P.d_recon + ((int64_t)(r / nb) * B + b0 + (r % nb)) * hs; });
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* row = mok ? lds_a + r16 * (hs + 4) : nullptr;
  const float* const ar[3] = {(mok && mi == 0) ? row : nullptr, (mok && mi == 1) ? row : nullptr, (mok && mi == 2) ? row : nullptr};
  const float* rw = P.rec_wT + (int64_t)wave * 16 * hs;
  const float* const bb[3] = {rw, rw + (int64_t)hs * hs, rw + (int64_t)2 * hs * hs};
  const int ld[3] = {hs, hs, hs};
  tile_mac_chain<3>(acc, ar, bb, ld, lane, lds_w + wave * 16 * WL_LD);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 4 * g + i;
    if (r < nmod) P.rec_part[((int64_t)(r / nb) * B + b0 + (r % nb)) * hs + col] = acc[i];
  }
}

// REG: the sentiment task's head (P.reg), an instance of its own like the forward stretch's
template <bool REG>
__global__ __launch_bounds__(FR_THREADS) void fused_bwd_c_kernel(FusedBwdC P) {
  __shared__ float red[2 * 8 * 128];
  __shared__ __attribute__((aligned(16))) float lds_a[6 * (128 + 4)];
  __shared__ __attribute__((aligned(16))) float lds_w[8 * 16 * WL_LD];
  const int nblk = (P.B + P.nb - 1) / P.nb;
  if ((int)blockIdx.x >= nblk) {                         // workgroup-uniform; only launched with rec_part
    const int rb0 = ((int)blockIdx.x - nblk) * P.nb;
    rec_part_rows(P, rb0, min(P.nb, P.B - rb0), lds_a, lds_w);
    return;
  }
  const int b0 = (int)blockIdx.x * P.nb;
  const int nb = min(P.nb, P.B - b0);
  const int NC = 6 + P.ncls, B = P.B, hs = P.hs;
  // heads backward: sigmoid' (and the dropout of the class scores) into d_logits
  for (int e = threadIdx.x; e < nb * NC; e += FR_THREADS) {
    const int b = b0 + e / NC, c = e % NC;
    P.d_logits[b * NC + c] = head_bwd_one<REG>(b, c, P.ncls, P.tcp, P.scores, P.d_tcp, P.d_scores, P.p_cls, P.seed, P.site_cls);
  }
  stage_sync();
  // d_hfused (nb, 6 hs) = d_logits (nb, NC) W_head (NC, 6 hs): a dozen terms per element
  const int W6 = 6 * hs;
  for (int e = threadIdx.x; e < nb * W6; e += FR_THREADS) {
    const int b = b0 + e / W6, n = e % W6;
    float acc = 0.f;
    for (int c = 0; c < NC; ++c) acc += P.d_logits[b * NC + c] * P.head_w[(int64_t)c * W6 + n];
    P.d_hfused[(int64_t)b * W6 + n] = acc;
  }
  stage_sync();
  // LayerNorm 2 backward over the token rows (s, b) of these samples
  ln_bwd_rows(P.ln2, S6K * nb, [&](int i) { return (i / nb) * B + b0 + (i % nb); }, red, pg_slot(P.pg_parts, b0, 0));
  pg_zero_rest(P.pg_parts, b0, nb, 0);
}

__global__ __launch_bounds__(FR_THREADS) void fused_bwd_a_kernel(FusedBwdA P) {
  __shared__ float red[2 * 8 * 128];
  __shared__ __attribute__((aligned(16))) float lds_a[LDS_A_FLOATS];
  __shared__ __attribute__((aligned(16))) float lds_w[8 * 16 * WL_LD];
  const int b0 = (int)blockIdx.x * P.nb;
  const int nb = min(P.nb, P.B - b0);
  const int B = P.B, hs = P.hs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int64_t BH = (int64_t)B * hs;
  int stamp_i = 0;
  auto stamp = [&]() { if (P.dbg && blockIdx.x == 0 && threadIdx.x == 0) P.dbg[stamp_i] = __builtin_readcyclecounter(); ++stamp_i; };
  stamp();
  flag_wait(P.wait_flag, P.wait_value, P.wait_err);
  // ---- d_x1 += sum of the feed-forward backward partials (slice order), for the token rows of these samples
  if (P.ffn_parts) {
    const int64_t MH = (int64_t)S6K * B * hs;
    auto off = [&](int gi) { const int i = gi / (hs / 4); return ((int64_t)(i / nb) * B + b0 + (i % nb)) * hs + 4 * (gi % (hs / 4)); };
    sum_parts_rows(P.ffn_parts, P.n_parts, MH, S6K * nb * (hs / 4), off, reinterpret_cast<f4*>(lds_a), [&](int gi, f4 t) {
      f4* d = reinterpret_cast<f4*>(P.d_x1 + off(gi));
      *d = *d + t;
    });
    stage_sync();
  }
  // ---- LayerNorm 1 backward: d_x6 += ..., d_attn_out
  ln_bwd_rows(P.ln1, S6K * nb, [&](int i) { return (i / nb) * B + b0 + (i % nb); }, red, pg_slot(P.pg_parts, b0, 1));
  pg_zero_rest(P.pg_parts, b0, nb, 1);
  stage_sync();
  stamp();
  // token-row tile: tile row r = j nb + bb  <->  global row j B + b0 + bb
  const int ntok = S6K * nb;                             // <= 12
  const bool rok = r16 < ntok;
  const int tj = rok ? r16 / nb : 0;
  const int col = wave * 16 + r16;                       // this lane's Bt row (output column): hs = 128 = 8 waves x 16
  // ---- d_ctx = d_attn_out W_out
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    stage_rows(lds_a, ntok, hs, [&](int r) { return P.d_attn_out + ((int64_t)(r / nb) * B + b0 + (r % nb)) * hs; });
    const float* const ar[1] = {rok ? lds_a + r16 * (hs + 4) : nullptr};
    const float* const bb[1] = {P.out_wT + (int64_t)wave * 16 * hs};
    const int ld[1] = {hs};
    tile_mac_chain<1>(acc, ar, bb, ld, lane, lds_w + wave * 16 * WL_LD);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * g + i;
      if (r < ntok) P.d_ctx[((int64_t)(r / nb) * B + b0 + (r % nb)) * hs + col] = acc[i];
    }
  }
  stage_sync();
  stamp();
  // ---- attention backward, one wave per (sample, head)
  for (int pr = wave; pr < nb * P.nhead; pr += FR_THREADS / 64)
    attn_bwd_hd64_one(P.qkv, P.probs, P.d_ctx, B, P.d_qkv, P.p_tf, P.seed, P.site_attn, P.nhead, (b0 + pr / P.nhead) * P.nhead + pr % P.nhead, lane);
  stage_sync();
  stamp();
  // ---- d_x6[j] = (d_x6[j] + d_qkv[j] W_in + d_recon[j % 3] W_rec[j % 3]) * s (1 - s)
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // (rows of the other two modalities multiply zeros in the per-modality products)
    // LDS: rows 0..ntok-1 = d_qkv rows (3 hs deep); behind them, at a stride of hs + 4, the d_recon row of every token row
    float* lds_r = lds_a + 12 * (3 * hs + 4);
    stage_rows(lds_a, ntok, 3 * hs, [&](int r) { return P.d_qkv + ((int64_t)(r / nb) * B + b0 + (r % nb)) * 3 * hs; });
    const float* qrow = rok ? lds_a + r16 * (3 * hs + 4) : nullptr;
    const float* wrow = P.in_wT + (int64_t)wave * 16 * 3 * hs;
    if (P.rec_part) {
      // the reconstruction term d_recon[j % 3] W_rec[j % 3] was made by workgroups of the stretch-C launch (fused_bwd_c_kernel): three
      // of this chain's six rounds are gone from it
      const float* const ar[3] = {qrow, qrow ? qrow + 128 : nullptr, qrow ? qrow + 256 : nullptr};
      const float* const bb[3] = {wrow, wrow + 128, wrow + 256};
      const int ld[3] = {3 * hs, 3 * hs, 3 * hs};
      tile_mac_chain<3>(acc, ar, bb, ld, lane, lds_w + wave * 16 * WL_LD);
    } else {
      stage_rows(lds_r, ntok, hs, [&](int r) { return P.d_recon + ((int64_t)((r / nb) % 3) * B + b0 + (r % nb)) * hs; });
      const float* rec_row = rok ? lds_r + r16 * (hs + 4) : nullptr;
      const float* const ar[6] = {qrow, qrow ? qrow + 128 : nullptr, qrow ? qrow + 256 : nullptr, (rok && tj % 3 == 0) ? rec_row : nullptr,
                                  (rok && tj % 3 == 1) ? rec_row : nullptr, (rok && tj % 3 == 2) ? rec_row : nullptr};
      const float* recw = P.rec_wT + (int64_t)wave * 16 * hs;
      const float* const bb[6] = {wrow, wrow + 128, wrow + 256, recw, recw + (int64_t)hs * hs, recw + (int64_t)2 * hs * hs};
      const int ld[6] = {3 * hs, 3 * hs, 3 * hs, hs, hs, hs};
      tile_mac_chain<6>(acc, ar, bb, ld, lane, lds_w + wave * 16 * WL_LD);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * g + i;
      if (r < ntok) {
        const int64_t o = ((int64_t)(r / nb) * B + b0 + (r % nb)) * hs + col;
        const float s = P.x6[o];
        float t = acc[i];
        if (P.rec_part) t += P.rec_part[((int64_t)((r / nb) % 3) * B + b0 + (r % nb)) * hs + col];
        P.d_x6[o] = (P.d_x6[o] + t) * (s * (1.f - s));
      }
    }
  }
  stage_sync();
  stamp();
  // ---- d_orig[i] += d_private[i] W_priv[i] + d_shared[i] W_shared; modality-row tile: tile row r = i nb + bb
  const int nmod = 3 * nb;
  const bool mok = r16 < nmod;
  const int mi = mok ? r16 / nb : 0;
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // LDS: rows 0..nmod-1 = d_private rows, rows nmod..2 nmod-1 = d_shared rows
    stage_rows(lds_a, 2 * nmod, hs, [&](int r) { return P.d_x6 + ((int64_t)((r / nmod) * 3 + (r % nmod) / nb) * B + b0 + (r % nb)) * hs; });
    const float* prow = mok ? lds_a + r16 * (hs + 4) : nullptr;
    const float* const ar[4] = {mok ? lds_a + (nmod + r16) * (hs + 4) : nullptr, (mok && mi == 0) ? prow : nullptr,
                                (mok && mi == 1) ? prow : nullptr, (mok && mi == 2) ? prow : nullptr};
    const float* pw = P.priv_wT + (int64_t)wave * 16 * hs;
    const float* const bb[4] = {P.sh_wT + (int64_t)wave * 16 * hs, pw, pw + (int64_t)hs * hs, pw + (int64_t)2 * hs * hs};
    const int ld[4] = {hs, hs, hs, hs};
    tile_mac_chain<4>(acc, ar, bb, ld, lane, lds_w + wave * 16 * WL_LD);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * g + i;
      if (r < nmod) {
        const int64_t o = ((int64_t)(r / nb) * B + b0 + (r % nb)) * hs + col;
        P.d_orig[o] += acc[i];
      }
    }
  }
  stage_sync();
  stamp();
  // ---- the three projection LayerNorms (with their activation) backward: d_z.  One wave per (modality, sample) row; a row's
  // dgamma / dbeta terms ARE that sample's partial (slot 2 + modality): stored, not added
  for (int i = wave; i < 3 * nb; i += FR_THREADS / 64) {
    const mmda_ln_bwd_args& a = P.lnp[i / nb];
    float dg[2] = {0.f, 0.f}, db[2] = {0.f, 0.f};
    ln_bwd_row<2>(a, b0 + i % nb, lane, dg, db);
    float* part = pg_slot(P.pg_parts, b0 + i % nb, 2 + i / nb);
    if (part) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = q * 64 + lane;
        part[c] = c < a.n ? dg[q] : 0.f;
        part[128 + c] = c < a.n ? db[q] : 0.f;
      }
    }
  }
  (void)BH;
  stamp();
}

// ---------------------------------------------------------------------------------------------------------------- forward stretches
// one round with the A row formed as the sum of two rows (private + shared)
__global__ __launch_bounds__(FR_THREADS) void fused_fwd_a_kernel(FusedFwdA P) {
  __shared__ __attribute__((aligned(16))) float lds_a[LDS_A_FLOATS];
  __shared__ __attribute__((aligned(16))) float lds_w[8 * 16 * WL_LD];
  // Roles (P.split_recon, small batches): the reconstruction reads x6 only and nothing of this stretch reads it, so it runs in
  // workgroups of its own -- [nblk, 2 nblk) -- beside the qkv -> attention -> out-projection -> LayerNorm chain instead of in front of it
  const int nblk = (P.B + P.nb - 1) / P.nb;
  const bool do_recon = !P.split_recon || (int)blockIdx.x >= nblk;
  const bool do_chain = !P.split_recon || (int)blockIdx.x < nblk;
  const int b0 = ((int)blockIdx.x % nblk) * P.nb;
  const int nb = min(P.nb, P.B - b0);
  const int B = P.B, hs = P.hs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int ntok = S6K * nb, nmod = 3 * nb;
  const bool rok = r16 < ntok;
  const bool mok = r16 < nmod;
  const int mi = mok ? r16 / nb : 0;
  const int col = wave * 16 + r16;
  // LDS: rows 0..ntok-1 = the x6 token rows; rows 12..12+nmod-1 = private + shared of (modality, sample)
  stage_rows(lds_a, ntok, hs, [&](int r) { return P.x6 + ((int64_t)(r / nb) * B + b0 + (r % nb)) * hs; });
  if (do_recon) {                                          // workgroup-uniform
  for (int e = threadIdx.x; e < nmod * (hs / 4); e += FR_THREADS) {
    const int r = e / (hs / 4), c = e % (hs / 4);
    const f4 a = *reinterpret_cast<const f4*>(lds_a + r * (hs + 4) + 4 * c), b2 = *reinterpret_cast<const f4*>(lds_a + (nmod + r) * (hs + 4) + 4 * c);
    *reinterpret_cast<f4*>(lds_a + (12 + r) * (hs + 4) + 4 * c) = a + b2;
  }
  __syncthreads();
  // ---- recon[i] = (x6[i] + x6[3 + i]) W_rec[i]^T + b_rec[i]: modality-row tile, three products into one accumulator
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* srow = mok ? lds_a + (12 + r16) * (hs + 4) : nullptr;
    const float* const ar[3] = {(mok && mi == 0) ? srow : nullptr, (mok && mi == 1) ? srow : nullptr, (mok && mi == 2) ? srow : nullptr};
    const float* rw = P.rec_w + (int64_t)wave * 16 * hs;
    const float* const bb[3] = {rw, rw + (int64_t)hs * hs, rw + (int64_t)2 * hs * hs};
    const int ld[3] = {hs, hs, hs};
    tile_mac_chain<3>(acc, ar, bb, ld, lane, lds_w + wave * 16 * WL_LD);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * g + i;
      if (r < nmod) {
        const int64_t o = ((int64_t)(r / nb) * B + b0 + (r % nb)) * hs + col;
        const float rv = acc[i] + P.rec_b[(r / nb) * hs + col];
        P.recon[o] = rv;
        if (P.d_recon) {
          const float gr = recon_seed(rv - P.orig[o], P.recon_inv_n, P.recon_scale);
          P.d_recon[o] = gr;
          P.d_orig[o] = 0.f - gr;
        }
      }
    }
  }
  }
  if (!do_chain) return;
  // ---- qkv = x6 W_in^T + b_in: token-row tile, 3 hs = 384 output columns = three passes of the eight waves
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int n = pass * 128 + col;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* const ar[1] = {rok ? lds_a + r16 * (hs + 4) : nullptr};
    const float* const bb[1] = {P.in_w + (int64_t)(pass * 128 + wave * 16) * hs};
    const int ld[1] = {hs};
    tile_mac_chain<1>(acc, ar, bb, ld, lane, lds_w + wave * 16 * WL_LD);
    const float bias = P.in_b[n];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * g + i;
      if (r < ntok) P.qkv[((int64_t)(r / nb) * B + b0 + (r % nb)) * 3 * hs + n] = acc[i] + bias;
    }
  }
  stage_sync();
  // ---- attention, one wave per (sample, head)
  for (int pr = wave; pr < nb * P.nhead; pr += FR_THREADS / 64)
    attn_fwd_hd64_one(P.qkv, B, P.ctx, P.probs, P.p_tf, P.seed, P.site_attn, P.nhead, (b0 + pr / P.nhead) * P.nhead + pr % P.nhead, lane);
  stage_sync();
  // ---- attn_out = ctx W_out^T + b_out
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    stage_rows(lds_a, ntok, hs, [&](int r) { return P.ctx + ((int64_t)(r / nb) * B + b0 + (r % nb)) * hs; });
    const float* const ar[1] = {rok ? lds_a + r16 * (hs + 4) : nullptr};
    const float* const bb[1] = {P.out_w + (int64_t)wave * 16 * hs};
    const int ld[1] = {hs};
    tile_mac_chain<1>(acc, ar, bb, ld, lane, lds_w + wave * 16 * WL_LD);
    const float bias = P.out_b[col];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * g + i;
      if (r < ntok) P.attn_out[((int64_t)(r / nb) * B + b0 + (r % nb)) * hs + col] = acc[i] + bias;
    }
  }
  stage_sync();
  // ---- LayerNorm 1 over the token rows
  for (int i = wave; i < ntok; i += FR_THREADS / 64) ln_fwd_row<2>(P.ln1, (i / nb) * B + b0 + (i % nb), lane);
}

// CLS_OPTS: the seed of the class-weighted / focal criterion (P.cls; loss_terms.h).  An instance of its own, so that the plain criterion's
// kernel -- the default step's -- is the code it was, registers and all.  REG: the sentiment task (P.reg), likewise.
template <bool CLS_OPTS, bool REG = false>
__global__ __launch_bounds__(FR_THREADS) void fused_fwd_c_kernel(FusedFwdC P) {
  __shared__ f4 sp[2 * 12 * 32];                         // sum_parts_rows: two halves x (<= 12 rows x 32 column groups)
  const int b0 = (int)blockIdx.x * P.nb;
  const int nb = min(P.nb, P.B - b0);
  const int B = P.B, hs = P.hs, NC = 6 + P.ncls, W6 = 6 * hs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // ---- f2 = sum of the feed-forward partials (slice order) + b2, for the token rows of these samples
  if (P.ffn_parts) {
    const int64_t MH = (int64_t)S6K * B * hs;
    auto off = [&](int gi) { const int i = gi / (hs / 4); return ((int64_t)(i / nb) * B + b0 + (i % nb)) * hs + 4 * (gi % (hs / 4)); };
    sum_parts_rows(P.ffn_parts, P.n_parts, MH, S6K * nb * (hs / 4), off, sp, [&](int gi, f4 t) {
      const float* b = P.b2 + 4 * (gi % (hs / 4));            // (a parameter: 4-byte aligned only)
      *reinterpret_cast<f4*>(P.f2 + off(gi)) = t + f4{b[0], b[1], b[2], b[3]};
    });
    stage_sync();
  }
  // ---- LayerNorm 2 over the token rows, written in the (B, 6 hs) layout the heads read
  for (int i = wave; i < S6K * nb; i += FR_THREADS / 64) ln_fwd_row<2>(P.ln2, (i / nb) * B + b0 + (i % nb), lane);
  stage_sync();
  // ---- logits = hfused W_head^T + b_head: a wave per (sample, output) pair, lanes along the 768-deep reduction; then the heads
  for (int e = wave; e < nb * NC; e += FR_THREADS / 64) {
    const int b = b0 + e / NC, c = e % NC;
    const float* x = P.hfused + (int64_t)b * W6;
    const float* w = P.head_w + (int64_t)c * W6;
    float acc = 0.f;
    for (int k = lane * 4; k < W6; k += 256) {
      const f4 xv = *reinterpret_cast<const f4*>(x + k), wv = *reinterpret_cast<const f4*>(w + k);
      acc += xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      const float z = acc + P.head_b[c];
      P.logits[b * NC + c] = z;
      head_fwd_one<REG>(z, b, c, P, [&](int k, float sc) {
        if (P.d_scores) {                                               // the classification loss's seed of class k
          const float yv = P.emo[b * P.ncls + k];
          float v, d;
          if constexpr (REG) reg_term(P.reg, sc, yv, v, d);
          else if constexpr (CLS_OPTS) cls_term(P.cls, sc, yv, k, v, d);
          else bce_plain(sc, yv, 1.f, v, d);
          P.d_scores[b * P.ncls + k] = d / B;
        }
      });
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- feed-forward pair
// See FusedFfnFwd.  Workgroup = (row block of FFN_RB rows, hidden slice of S = 32 units), 8 waves.
//   product 1 (K = hs = 128): FFN_RB / 16 row tiles x 2 column tiles; wave w keeps the weight fragments of column tile w >> 2 in registers
//     and walks row tiles (w & 3), + 4, ... with A from the LDS image of the row block
//   product 2 (K = S): FFN_RB / 16 row tiles x 8 column tiles; wave w keeps the fragments of output columns 16 w.. and walks all row tiles with A
//     from the LDS image of product 1's result
constexpr int FFN_RB = 48, FFN_S = 32;       // rows per workgroup (launch time at B=32: 21 us with 192, 12.7 with 96 or 48; B=256 step 2.227 / 2.210 / 2.200 ms)
constexpr int FFN_LDS_X = FFN_RB * (128 + 4), FFN_LDS_H = FFN_RB * (FFN_S + 4);

struct FfnGeom { int rb0, nrows, j; };

// the two products on LDS images: xs (rows, hs + 4) -> hs_ (rows, S + 4) via epi1(row, unit, value) -> partial via store2(row, col, value)
template <typename Epi1, typename Store2>
__device__ __forceinline__ void ffn_two_products(const float* xs, float* hs_, const float* __restrict__ b1rows /* S rows x 128, K-major */,
                                                 int ldb1, const float* __restrict__ b2rows /* 128 rows x S, K-major */, int ldb2,
                                                 Epi1 epi1, Store2 store2) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  {
    // product 1: this wave's column tile ct, weights of its 16 units for the whole K = 128 in registers
    const int ct = wave >> 2;
    f4 bw[8];
    const float* brow = b1rows + (int64_t)(ct * 16 + r16) * ldb1;
#pragma unroll
    for (int c = 0; c < 8; ++c) bw[c] = *reinterpret_cast<const f4*>(brow + 16 * c + 4 * g);
#pragma unroll
    for (int q = 0; q < (FFN_RB / 16 + 3) / 4; ++q) {
      const int rt = (wave & 3) + 4 * q;
      if (rt >= FFN_RB / 16) break;                      // wave-uniform
      const float* arow = xs + (rt * 16 + r16) * (128 + 4);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const f4 a = *reinterpret_cast<const f4*>(arow + 16 * c + 4 * g);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bw[c][s], acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = rt * 16 + 4 * g + i, unit = ct * 16 + r16;
        hs_[row * (FFN_S + 4) + unit] = epi1(row, unit, acc[i]);
      }
    }
  }
  __syncthreads();
  {
    // product 2: output columns 16 wave .. + 15, K = S = 32 (two chunks)
    f4 bw[2];
    const float* brow = b2rows + (int64_t)(wave * 16 + r16) * ldb2;
#pragma unroll
    for (int c = 0; c < 2; ++c) bw[c] = *reinterpret_cast<const f4*>(brow + 16 * c + 4 * g);
#pragma unroll
    for (int rt = 0; rt < FFN_RB / 16; ++rt) {
      const float* arow = hs_ + (rt * 16 + r16) * (FFN_S + 4);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const f4 a = *reinterpret_cast<const f4*>(arow + 16 * c + 4 * g);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bw[c][s], acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) store2(rt * 16 + 4 * g + i, wave * 16 + r16, acc[i]);
    }
  }
}

// rows [rb0, rb0 + nrows) of a (M, 128) matrix into the LDS image (rows past M as zeros)
__device__ __forceinline__ void ffn_stage_x(float* xs, const float* __restrict__ X, int rb0, int M) {
  constexpr int PER = FFN_RB * 32 / FR_THREADS;         // float4 per thread, all loads issued before the first LDS store
  f4 v[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = threadIdx.x + u * FR_THREADS, r = e >> 5, c = e & 31;
    v[u] = *reinterpret_cast<const f4*>(X + (int64_t)min(rb0 + r, M - 1) * 128 + 4 * c);
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = threadIdx.x + u * FR_THREADS, r = e >> 5, c = e & 31;
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f4*>(xs + r * (128 + 4) + 4 * c) = (rb0 + r < M) ? v[u] : z;
  }
  __syncthreads();
}

__global__ __launch_bounds__(FR_THREADS) void fused_ffn_fwd_kernel(FusedFfnFwd P) {
  extern __shared__ __attribute__((aligned(16))) float ffn_lds[];
  float* xs = ffn_lds; float* hs_ = ffn_lds + FFN_LDS_X;
  const int nsl = P.F / FFN_S;
  const int j = (int)blockIdx.x % nsl, rb0 = ((int)blockIdx.x / nsl) * FFN_RB;
  ffn_stage_x(xs, P.x1, rb0, P.M);
  float* part = P.parts + (int64_t)j * P.M * P.hs;
  ffn_two_products(xs, hs_, P.w1 + (int64_t)j * FFN_S * P.hs, P.hs, P.w2 + (int64_t)j * FFN_S, P.F,
    [&](int row, int unit, float v) {
      const int m = rb0 + row, n = j * FFN_S + unit;
      v += P.b1[n];
      v = fmaxf(v, 0.f);
      if (P.p > 0.f) v *= drop_mul(P.p, P.seed, P.site, (uint64_t)m * P.F + n);
      if (m < P.M) P.f1[(int64_t)m * P.F + n] = v; else v = 0.f;
      return v;
    },
    [&](int row, int col, float v) { if (rb0 + row < P.M) part[(int64_t)(rb0 + row) * P.hs + col] = v; });
}

__global__ __launch_bounds__(FR_THREADS) void fused_ffn_bwd_kernel(FusedFfnBwd P) {
  extern __shared__ __attribute__((aligned(16))) float ffn_lds[];
  float* xs = ffn_lds; float* hs_ = ffn_lds + FFN_LDS_X;
  const int nsl = P.F / FFN_S;
  const int j = (int)blockIdx.x % nsl, rb0 = ((int)blockIdx.x / nsl) * FFN_RB;
  ffn_stage_x(xs, P.d_f2, rb0, P.M);
  float* part = P.parts + (int64_t)j * P.M * P.hs;
  ffn_two_products(xs, hs_, P.l2_wT + (int64_t)j * FFN_S * P.hs, P.hs, P.l1_wT + (int64_t)j * FFN_S, P.F,
    [&](int row, int unit, float v) {
      const int m = rb0 + row, n = j * FFN_S + unit;
      if (m >= P.M) return 0.f;
      v *= (P.f1[(int64_t)m * P.F + n] > 0.f) ? P.gate_scale : 0.f;      // f1 is stored post-relu, post-dropout
      P.d_f1[(int64_t)m * P.F + n] = v;
      return v;
    },
    [&](int row, int col, float v) { if (rb0 + row < P.M) part[(int64_t)(rb0 + row) * P.hs + col] = v; });
}

}  // namespace

int mmda_fused_ffn_fwd(const FusedFfnFwd* a, void* stream) {
  if (!a || a->M <= 0 || a->hs != 128 || a->S != FFN_S || a->F <= 0 || (a->F % FFN_S)) return MMDA_EINVAL;
  const int lds = (FFN_LDS_X + FFN_LDS_H) * 4;
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fused_ffn_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds); attr = true; }
  hipLaunchKernelGGL(fused_ffn_fwd_kernel, dim3((a->F / FFN_S) * ceil_div(a->M, FFN_RB)), dim3(FR_THREADS), lds, (hipStream_t)stream, *a);
  MMDA_CHECK_LAUNCH("mmda_fused_ffn_fwd");
  return MMDA_OK;
}

int mmda_fused_ffn_bwd(const FusedFfnBwd* a, void* stream) {
  if (!a || a->M <= 0 || a->hs != 128 || a->S != FFN_S || a->F <= 0 || (a->F % FFN_S)) return MMDA_EINVAL;
  const int lds = (FFN_LDS_X + FFN_LDS_H) * 4;
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fused_ffn_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds); attr = true; }
  hipLaunchKernelGGL(fused_ffn_bwd_kernel, dim3((a->F / FFN_S) * ceil_div(a->M, FFN_RB)), dim3(FR_THREADS), lds, (hipStream_t)stream, *a);
  MMDA_CHECK_LAUNCH("mmda_fused_ffn_bwd");
  return MMDA_OK;
}

int mmda_fused_fwd_a(const FusedFwdA* a, void* stream) {
  if (!a || a->B <= 0 || a->nb <= 0 || a->nb > 2 || a->hs != 128 || a->nhead != 2 || a->ln1.n != 128) return MMDA_EINVAL;
  if (a->d_recon && (!a->orig || !a->d_orig)) return MMDA_EINVAL;
  // (the reconstruction in workgroups of its own while both roles together leave the chip half empty; MMDA_FUSED_SPLIT=0: never)
  static const int split_on = mmda_env_int("MMDA_FUSED_SPLIT", 1);
  FusedFwdA f = *a;
  const int nblk = ceil_div(a->B, a->nb);
  f.split_recon = (split_on && nblk <= 64) ? 1 : 0;
  hipLaunchKernelGGL(fused_fwd_a_kernel, dim3(f.split_recon ? 2 * nblk : nblk), dim3(FR_THREADS), 0, (hipStream_t)stream, f);
  MMDA_CHECK_LAUNCH("mmda_fused_fwd_a");
  return MMDA_OK;
}

int mmda_fused_fwd_c(const FusedFwdC* a, void* stream) {
  if (!a || a->B <= 0 || a->nb <= 0 || a->nb > 2 || a->hs != 128 || a->ln2.n != 128 || (a->d_scores && !a->emo)) return MMDA_EINVAL;
  if (!reg_valid(a->reg) || (a->reg != REG_NONE && !cls_plain(a->cls))) return MMDA_EINVAL;
  const bool opts = a->d_scores && !cls_plain(a->cls);
  void (*const reg_kernel)(FusedFwdC) = fused_fwd_c_kernel<false, true>;        // (a name without a comma for the launch macro)
  hipLaunchKernelGGL(a->reg != REG_NONE ? reg_kernel : opts ? fused_fwd_c_kernel<true> : fused_fwd_c_kernel<false>, dim3(ceil_div(a->B, a->nb)), dim3(FR_THREADS), 0,
                     (hipStream_t)stream, *a);
  MMDA_CHECK_LAUNCH("mmda_fused_fwd_c");
  return MMDA_OK;
}

// parameter gradients of the five LayerNorms: partials of the samples added in sample order (sixteen loads in flight at a time)
struct FusedPgOut { float* dgamma[FUSED_PG_SLOTS]; float* dbeta[FUSED_PG_SLOTS]; };
__global__ __launch_bounds__(256) void fused_pg_finish_kernel(const float* __restrict__ parts, int B, int hs, FusedPgOut out) {
  // sixteen threads per output (slot k, gamma | beta, column c): each adds every sixteenth sample's partial, the sub-sums in lane order
  __shared__ float sub[256];
  const int e = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  const bool ok = e < FUSED_PG_SLOTS * 256;
  const int k = ok ? e / 256 : 0, which = (e % 256) / 128, c = e % 128;
  const float* p = parts + (int64_t)k * 256 + which * 128 + c;
  float acc = 0.f;
  if (ok) {
    const int64_t st = (int64_t)FUSED_PG_SLOTS * 256;
    int b = j;
    for (; b + 7 * 16 < B; b += 8 * 16) {                  // eight loads in flight
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(b + 16 * u) * st];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; b < B; b += 16) acc += p[b * st];
  }
  sub[threadIdx.x] = acc;
  __syncthreads();
  float* dst = which ? out.dbeta[k] : out.dgamma[k];
  if (ok && j == 0 && dst && c < hs) {
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) t += sub[(threadIdx.x & ~15) + u];
    dst[c] += t;
  }
}

int mmda_fused_pg_finish(const float* pg_parts, int B, int hs, float* const* dgamma, float* const* dbeta, void* stream) {
  if (!pg_parts || B <= 0 || hs != 128 || !dgamma || !dbeta) return MMDA_EINVAL;
  FusedPgOut out;
  for (int k = 0; k < FUSED_PG_SLOTS; ++k) { out.dgamma[k] = dgamma[k]; out.dbeta[k] = dbeta[k]; }
  hipLaunchKernelGGL(fused_pg_finish_kernel, dim3(FUSED_PG_SLOTS * 256 / 16), dim3(256), 0, (hipStream_t)stream, pg_parts, B, hs, out);
  MMDA_CHECK_LAUNCH("mmda_fused_pg_finish");
  return MMDA_OK;
}

int mmda_fused_bwd_c(const FusedBwdC* a, void* stream) {
  if (!a || a->B <= 0 || a->nb <= 0 || a->hs != 128 || a->ln2.n != 128) return MMDA_EINVAL;
  if ((a->ln2.dgamma || a->ln2.dbeta) && !a->pg_parts) return MMDA_EINVAL;       // parameter gradients go through the partials
  if (a->rec_part && (!a->d_recon || !a->rec_wT || a->nb > 2)) return MMDA_EINVAL;
  if (!reg_valid(a->reg)) return MMDA_EINVAL;
  hipLaunchKernelGGL(a->reg != REG_NONE ? fused_bwd_c_kernel<true> : fused_bwd_c_kernel<false>, dim3(ceil_div(a->B, a->nb) * (a->rec_part ? 2 : 1)), dim3(FR_THREADS), 0, (hipStream_t)stream, *a);
  MMDA_CHECK_LAUNCH("mmda_fused_bwd_c");
  return MMDA_OK;
}

static unsigned long long* g_fr_dbg = nullptr;
extern "C" int mmda_debug_set_fused_stamps(void* device_buffer) { g_fr_dbg = (unsigned long long*)device_buffer; return MMDA_OK; }

int mmda_fused_bwd_a(const FusedBwdA* a, void* stream) {
  if (!a || a->B <= 0 || a->nb <= 0 || a->nb > 2 || a->hs != 128 || a->nhead != 2) return MMDA_EINVAL;
  // (every row of this stretch is hs wide: the GEMM stages read and write 128 columns of what the LayerNorms leave)
  if (a->ln1.n != 128 || a->lnp[0].n != 128 || a->lnp[1].n != 128 || a->lnp[2].n != 128) return MMDA_EINVAL;
  if ((a->ln1.dgamma || a->ln1.dbeta || a->lnp[0].dgamma || a->lnp[0].dbeta) && !a->pg_parts) return MMDA_EINVAL;
  FusedBwdA P = *a;
  P.dbg = g_fr_dbg;
  hipLaunchKernelGGL(fused_bwd_a_kernel, dim3(ceil_div(a->B, a->nb)), dim3(FR_THREADS), 0, (hipStream_t)stream, P);
  MMDA_CHECK_LAUNCH("mmda_fused_bwd_a");
  return MMDA_OK;
}

// tests/ and tools/ only (fused_rows.h): each launch alone, and the struct sizes the ctypes mirrors of tests/fused_rows_cases.py must have
extern "C" int mmda_debug_fused_fwd_a(const FusedFwdA* a, void* stream) { return mmda_fused_fwd_a(a, stream); }
extern "C" int mmda_debug_fused_ffn_fwd(const FusedFfnFwd* a, void* stream) { return mmda_fused_ffn_fwd(a, stream); }
extern "C" int mmda_debug_fused_fwd_c(const FusedFwdC* a, void* stream) { return mmda_fused_fwd_c(a, stream); }
extern "C" int mmda_debug_fused_bwd_c(const FusedBwdC* a, void* stream) { return mmda_fused_bwd_c(a, stream); }
extern "C" int mmda_debug_fused_ffn_bwd(const FusedFfnBwd* a, void* stream) { return mmda_fused_ffn_bwd(a, stream); }
extern "C" int mmda_debug_fused_bwd_a(const FusedBwdA* a, void* stream) { return mmda_fused_bwd_a(a, stream); }
extern "C" int mmda_debug_fused_pg_finish(const float* pg_parts, int B, int hs, float* const* dgamma, float* const* dbeta, void* stream) {
  return mmda_fused_pg_finish(pg_parts, B, hs, dgamma, dbeta, stream);
}
extern "C" int mmda_debug_fused_sizeof(int which) {
  switch (which) {
    case 0: return (int)sizeof(FusedFwdA);
    case 1: return (int)sizeof(FusedFwdC);
    case 2: return (int)sizeof(FusedBwdC);
    case 3: return (int)sizeof(FusedBwdA);
    case 4: return (int)sizeof(FusedFfnFwd);
    case 5: return (int)sizeof(FusedFfnBwd);
    case 6: return (int)sizeof(ClsTerm);
    default: return -1;
  }
}
