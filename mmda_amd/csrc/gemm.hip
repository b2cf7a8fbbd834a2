// Generic LDS-tiled MFMA GEMM for gfx950: fp32 data in HBM, f32 MFMA (exact) or bf16 MFMA (fp32 accumulate).
// One kernel serves every nn.Linear forward (NT), its input gradient (NN) and weight gradient (TN) on the path;
// operands whose inner dimension is 35/74/140/296/300 are handled by bounds-checked staging (zero fill).
//
// Tile 64x64x32, 256 threads = 4 waves (2x2), each wave a 32x32 sub-tile = 2x2 MFMA 16x16 accumulators.
#include "common.h"
#include "internal.h"
#include "splitk.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 32;
constexpr int LDS_F32_LD = 34;   // floats per LDS row: (2*row + k) % 32 distinct for the 16x16x4 operand reads
constexpr int LDS_BF16_LD = 40;  // shorts per LDS row (80 B, 16-B aligned rows for ds_read_b128)

template <int MODE, int PF>
__device__ __forceinline__ void gemm_body(const mmda_gemm_args& g, int splitk, unsigned char* smem, int bx, int by, int bzz,
                                          float* slab, int ldn) {
  float* As_f = reinterpret_cast<float*>(smem);
  float* Bs_f = As_f + BM * LDS_F32_LD;
  unsigned short* As_h = reinterpret_cast<unsigned short*>(smem);
  unsigned short* Bs_h = As_h + BM * LDS_BF16_LD;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int row0 = by * BM, col0 = bx * BN;
  const int64_t bz = bzz / splitk;
  const int sp = bzz % splitk;
  const float* A = g.A + bz * g.strideA;
  const float* A2 = g.A2 ? g.A2 + bz * g.strideA : nullptr;
  const float* Bm = g.B + bz * g.strideB;
  float* C = g.C + bz * g.strideC;
  const int M = g.M, N = g.N, K = g.K;

  // per-thread staging coordinates (fixed across k-tiles)
  int a_r[8], a_k[8], b_r[8], b_k[8];
  int64_t a_row_off_c[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int e = tid + 256 * i;
    if (g.transA) { a_r[i] = e & 63; a_k[i] = e >> 6; } else { a_r[i] = e >> 5; a_k[i] = e & 31; }
    if (g.transB) { b_r[i] = e >> 5; b_k[i] = e & 31; } else { b_r[i] = e & 63; b_k[i] = e >> 6; }
    int m = row0 + a_r[i];
    int64_t src = min(m, M - 1);
    if (g.gather) src = g.gather[min(m, M - 1)];
    a_row_off_c[i] = src;                               // (clamped: rows past M load a valid row and are zeroed at the LDS store)
  }

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Register staging.  Every load is UNCONDITIONAL from a clamped (always valid) address and the zero fill of the out-of-range
  // elements happens when the value is stored to LDS: a load under a lane-dependent branch costs a full `s_waitcnt vmcnt(0)` each --
  // sixteen serialised memory latencies per k-tile (the fusion block's weight-gradient launch took 232 us at B = 256 that way).
  float rap[PF][8], rbp[PF][8];
  unsigned okp[PF];                                     // bit i: A element i in range; bit 8 + i: B element i; bit 16 + i: B element i is the ones column
  auto load_tile = [&](float (&ra)[8], float (&rb)[8], unsigned& ok, int k0) {
    ok = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = row0 + a_r[i], k = k0 + a_k[i];
      const bool va = m < M && k < K;
      const int kc = max(0, min(k, K - 1));
      const int64_t off = g.transA ? (int64_t)kc * g.lda + min(m, M - 1) : a_row_off_c[i] * g.lda + kc;
      float v = A[off];
      if (A2) v += A2[off];                              // (kernel-uniform)
      ra[i] = v;
      ok |= va ? (1u << i) : 0u;
      const int n = col0 + b_r[i];
      const int kb = k0 + b_k[i];
      const bool vb = n < N && kb < K;
      const int nc = min(n, N - 1), kbc = max(0, min(kb, K - 1));
      rb[i] = g.transB ? Bm[(int64_t)nc * g.ldb + kbc] : Bm[(int64_t)kbc * g.ldb + nc];
      ok |= vb ? (1u << (8 + i)) : 0u;
      ok |= (g.bias_grad && n == N && kb < K) ? (1u << (16 + i)) : 0u;      // virtual all-ones column: its output is the bias gradient
    }
  };
  auto store_tile = [&](const float (&ra)[8], const float (&rb)[8], unsigned ok) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float av = (ok >> i) & 1u ? ra[i] : 0.f;
      const float bv = (ok >> (16 + i)) & 1u ? 1.0f : ((ok >> (8 + i)) & 1u ? rb[i] : 0.f);
      if (MODE == MMDA_BF16) {
        As_h[a_r[i] * LDS_BF16_LD + a_k[i]] = f2bf(av);
        Bs_h[b_r[i] * LDS_BF16_LD + b_k[i]] = f2bf(bv);
      } else {
        As_f[a_r[i] * LDS_F32_LD + a_k[i]] = av;
        Bs_f[b_r[i] * LDS_F32_LD + b_k[i]] = bv;
      }
    }
  };

  // split-K: this block reduces k-tiles [kt0, kt1); its raw partial tile goes into a slab of its own and the reduce launch behind
  // this one sums the slabs in slice order (splitk.h): no float atomics, identical bits on every run
  const int nk_all = (K + BK - 1) / BK;
  const int per = (nk_all + splitk - 1) / splitk;
  const int kt0 = sp * per;
  const int nk = min(nk_all, kt0 + per);
  if (splitk > 1 && kt0 >= nk) return;
  // PF == 1: one k-tile of register prefetch under the MFMAs (long k-loops, many workgroups in flight).
  // PF == 4: tiny problems (<= 4 k-tiles per block, a handful of blocks): issue ALL global loads up front so the block pays
  //          one first-touch memory latency instead of one per k-tile.
  if (PF > 1) {
#pragma unroll
    for (int p = 0; p < PF; ++p)
      if (kt0 + p < nk) load_tile(rap[p], rbp[p], okp[p], (kt0 + p) * BK);
  } else {
    load_tile(rap[0], rbp[0], okp[0], kt0 * BK);
  }
#pragma unroll 1
  for (int kt = kt0; kt < nk; ++kt) {
    __syncthreads();            // previous tile's fragment reads are done
    if (PF > 1) {
      const int p = kt - kt0;
      if (p == 0) store_tile(rap[0], rbp[0], okp[0]);
      else if (p == 1) store_tile(rap[PF > 1 ? 1 : 0], rbp[PF > 1 ? 1 : 0], okp[PF > 1 ? 1 : 0]);
      else if (p == 2) store_tile(rap[PF > 2 ? 2 : 0], rbp[PF > 2 ? 2 : 0], okp[PF > 2 ? 2 : 0]);
      else store_tile(rap[PF > 3 ? 3 : 0], rbp[PF > 3 ? 3 : 0], okp[PF > 3 ? 3 : 0]);
    } else {
      store_tile(rap[0], rbp[0], okp[0]);
    }
    __syncthreads();
    if (PF == 1 && kt + 1 < nk) load_tile(rap[0], rbp[0], okp[0], (kt + 1) * BK);   // global loads fly under the MFMAs below
    const int fr = lane & 15, fq = lane >> 4;
    if (MODE == MMDA_BF16) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *reinterpret_cast<const bf16x8*>(&As_h[(wm * 32 + i * 16 + fr) * LDS_BF16_LD + fq * 8]);
        b[i] = *reinterpret_cast<const bf16x8*>(&Bs_h[(wn * 32 + i * 16 + fr) * LDS_BF16_LD + fq * 8]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk) {
        float a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = As_f[(wm * 32 + i * 16 + fr) * LDS_F32_LD + kk * 4 + fq];
          b[i] = Bs_f[(wn * 32 + i * 16 + fr) * LDS_F32_LD + kk * 4 + fq];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
  }

  // epilogue: C/D fragment map col = lane&15, row = (lane>>4)*4 + reg
  if (splitk > 1) {                // host guarantees: no act/dropout/gate; slab = [batch][slice][M][ldn]
    float* S = slab + ((int64_t)bz * splitk + sp) * M * ldn;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = col0 + wn * 32 + j * 16 + (lane & 15);
        if (n >= ldn) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = row0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
          if (m < M) S[(int64_t)m * ldn + n] = acc[i][j][r];
        }
      }
    return;
  }
  const float* bias = g.bias ? g.bias + bz * g.strideBias : nullptr;
  const float* bias2 = g.bias2 ? g.bias2 + bz * g.strideBias : nullptr;
  const float alpha = g.alpha == 0.f ? 1.f : g.alpha;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int n = col0 + wn * 32 + j * 16 + (lane & 15);
      if (g.bias_grad && n == N) {                           // column sums of A (= dY) into the bias gradient(s): one writer per entry
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int m = row0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
          if (m < M) {
            g.bias_grad[bz * g.strideBias + m] += acc[i][j][r];
            if (g.bias_grad2) g.bias_grad2[bz * g.strideBias + m] += acc[i][j][r];
          }
        }
        continue;
      }
      if (n >= N) continue;
      float bsum = 0.f;
      if (bias) bsum += bias[n];
      if (bias2) bsum += bias2[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int m = row0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
        if (m >= M) continue;
        int64_t ci = (int64_t)m * g.ldc + n;
        float v = alpha * acc[i][j][r] + bsum;
        if (g.accumulate) v += C[ci];
        v = act_fwd(g.act, v);
        if (g.drop_p > 0.f) v *= drop_mul(g.drop_p, g.drop_seed, g.drop_site, ((uint64_t)bz * M + m) * N + n);
        if (g.gate) v *= (g.gate[bz * g.strideC + (int64_t)m * g.ldgate + n] > 0.f) ? g.gate_scale : 0.f;
        C[ci] = v;
      }
    }
}


template <int MODE, int PF>
__global__ __launch_bounds__(256) void gemm_kernel(mmda_gemm_args g, int splitk, float* slab, int ldn) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BM * LDS_F32_LD * 4];
  gemm_body<MODE, PF>(g, splitk, smem, blockIdx.x, blockIdx.y, blockIdx.z, slab, ldn);
}

// Grouped launch: up to GROUP_MAX independent GEMMs (different shapes, layouts, modes) in ONE grid, so that the many small
// LSTM gradient GEMMs of the three modalities fill the chip together instead of running one after another at a few dozen
// workgroups each.  blockIdx.x -> (problem, tile) through the prefix table.
constexpr int GROUP_MAX = 16;
struct GroupLaunch {
  mmda_gemm_args p[GROUP_MAX];
  int start[GROUP_MAX + 1];
  int tx[GROUP_MAX], ty[GROUP_MAX], splitk[GROUP_MAX];
  float* slab[GROUP_MAX];
  int ldn[GROUP_MAX];
  int n;
};
__global__ __launch_bounds__(256) void gemm_grouped_kernel(GroupLaunch G) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BM * LDS_F32_LD * 4];
  int i = 0;
#pragma unroll
  for (int k = 1; k < GROUP_MAX; ++k)
    if (k < G.n && (int)blockIdx.x >= G.start[k]) i = k;
  const int local = blockIdx.x - G.start[i];
  const int bx = local % G.tx[i], by = (local / G.tx[i]) % G.ty[i], bzz = local / (G.tx[i] * G.ty[i]);
  const mmda_gemm_args g = G.p[i];      // one copy into SGPRs; indexing the kernarg array inside the k-loop would re-load fields
  const int sk = G.splitk[i];
  if (g.mode == MMDA_BF16) gemm_body<MMDA_BF16, 1>(g, sk, smem, bx, by, bzz, G.slab[i], G.ldn[i]);
  else gemm_body<MMDA_F32, 1>(g, sk, smem, bx, by, bzz, G.slab[i], G.ldn[i]);
}

// ------------------------------------------------------------------------------------------------ 128x128 bf16 tile
// The LSTM-sized GEMMs (M = T*B rows, N/K in {300, 600, 1200, 2400}) with 16-byte fp32 staging loads, a 128x128x32 tile
// and a 64x64 sub-tile per wave: 16 MFMA 16x16x32 per wave and k-tile against 8 ds_read_b128 (the 64x64 kernel above
// issues 4 MFMAs per 4 reads and 16 scalar loads per thread).  Requires 16-byte aligned rows (leading dims % 4 == 0,
// K % 4 == 0, M % 4 == 0 for transA / N % 4 == 0 for !transB) and a plain epilogue; the host picks it when that holds.
constexpr int TM = 128, TN = 128;

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm128_bf16_kernel(mmda_gemm_args g, int splitk, float* slab, int ldn) {
  __shared__ __attribute__((aligned(16))) unsigned short As[TM * LDS_BF16_LD];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[TN * LDS_BF16_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int row0 = blockIdx.y * TM, col0 = blockIdx.x * TN;
  const int64_t bz = blockIdx.z / splitk;
  const int sp = blockIdx.z % splitk;
  const float* A = g.A + bz * g.strideA;
  const float* Bm = g.B + bz * g.strideB;
  float* C = g.C + bz * g.strideC;
  const int M = g.M, N = g.N, K = g.K;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  float4 ra[4], rb[4];
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gi = tid + 256 * i;
      float4 v = float4{0.f, 0.f, 0.f, 0.f};
      if (!TA) {                       // A (M,K): 8 groups of 4 k per row
        const int r = gi >> 3, k = k0 + (gi & 7) * 4;
        if (row0 + r < M && k < K) v = *reinterpret_cast<const float4*>(A + (int64_t)(row0 + r) * g.lda + k);
      } else {                         // A (K,M): 32 groups of 4 m per k-row
        const int k = k0 + (gi >> 5), m = row0 + (gi & 31) * 4;
        if (k < K && m < M) v = *reinterpret_cast<const float4*>(A + (int64_t)k * g.lda + m);
      }
      ra[i] = v;
      float4 u = float4{0.f, 0.f, 0.f, 0.f};
      if (TB) {                        // B (N,K)
        const int r = gi >> 3, k = k0 + (gi & 7) * 4;
        if (col0 + r < N && k < K) u = *reinterpret_cast<const float4*>(Bm + (int64_t)(col0 + r) * g.ldb + k);
      } else {                         // B (K,N)
        const int k = k0 + (gi >> 5), n = col0 + (gi & 31) * 4;
        if (k < K && n < N) u = *reinterpret_cast<const float4*>(Bm + (int64_t)k * g.ldb + n);
      }
      rb[i] = u;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gi = tid + 256 * i;
      if (!TA) {
        const int r = gi >> 3, k = (gi & 7) * 4;
        uint2 p; p.x = f2bf(ra[i].x) | ((unsigned)f2bf(ra[i].y) << 16); p.y = f2bf(ra[i].z) | ((unsigned)f2bf(ra[i].w) << 16);
        *reinterpret_cast<uint2*>(&As[r * LDS_BF16_LD + k]) = p;
      } else {
        const int k = gi >> 5, m = (gi & 31) * 4;
        As[(m + 0) * LDS_BF16_LD + k] = f2bf(ra[i].x); As[(m + 1) * LDS_BF16_LD + k] = f2bf(ra[i].y);
        As[(m + 2) * LDS_BF16_LD + k] = f2bf(ra[i].z); As[(m + 3) * LDS_BF16_LD + k] = f2bf(ra[i].w);
      }
      if (TB) {
        const int r = gi >> 3, k = (gi & 7) * 4;
        uint2 p; p.x = f2bf(rb[i].x) | ((unsigned)f2bf(rb[i].y) << 16); p.y = f2bf(rb[i].z) | ((unsigned)f2bf(rb[i].w) << 16);
        *reinterpret_cast<uint2*>(&Bs[r * LDS_BF16_LD + k]) = p;
      } else {
        const int k = gi >> 5, n = (gi & 31) * 4;
        Bs[(n + 0) * LDS_BF16_LD + k] = f2bf(rb[i].x); Bs[(n + 1) * LDS_BF16_LD + k] = f2bf(rb[i].y);
        Bs[(n + 2) * LDS_BF16_LD + k] = f2bf(rb[i].z); Bs[(n + 3) * LDS_BF16_LD + k] = f2bf(rb[i].w);
      }
    }
  };

  const int nk_all = (K + BK - 1) / BK;
  const int per = (nk_all + splitk - 1) / splitk;
  const int kt0 = sp * per;
  const int nk = min(nk_all, kt0 + per);
  if (splitk > 1 && kt0 >= nk) return;
  load_tile(kt0 * BK);
  const int fr = lane & 15, fq = lane >> 4;
  for (int kt = kt0; kt < nk; ++kt) {
    __syncthreads();
    store_tile();
    __syncthreads();
    if (kt + 1 < nk) load_tile((kt + 1) * BK);
    bf16x8 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = *reinterpret_cast<const bf16x8*>(&As[(wm * 64 + i * 16 + fr) * LDS_BF16_LD + fq * 8]);
      b[i] = *reinterpret_cast<const bf16x8*>(&Bs[(wn * 64 + i * 16 + fr) * LDS_BF16_LD + fq * 8]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
  }

  const float* bias = g.bias ? g.bias + bz * g.strideBias : nullptr;
  const float* bias2 = g.bias2 ? g.bias2 + bz * g.strideBias : nullptr;
  const float alpha = g.alpha == 0.f ? 1.f : g.alpha;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = col0 + wn * 64 + j * 16 + (lane & 15);
      if (n >= N) continue;
      float bsum = 0.f;
      if (bias) bsum += bias[n];
      if (bias2) bsum += bias2[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = row0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
        if (m >= M) continue;
        const int64_t ci = (int64_t)m * g.ldc + n;
        if (splitk > 1) { slab[(((int64_t)bz * splitk + sp) * M + m) * ldn + n] = acc[i][j][r]; continue; }
        float v = alpha * acc[i][j][r] + bsum;
        if (g.accumulate) v += C[ci];
        C[ci] = v;
      }
    }
}

// column sums of X (M, N) added into out (and out2): stage 1 writes one partial row per row block, stage 2 adds the partials of a
// column in block order (no atomics: the same bits on every run)
__global__ void colsum_kernel(const float* __restrict__ X, int ld, int M, int N, float* part, int rows_per_block) {
  __shared__ float red[4][64];
  int c = blockIdx.x * 64 + (threadIdx.x & 63);
  int rg = threadIdx.x >> 6;
  int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
  float s = 0.f;
  if (c < N)
    for (int r = r0 + rg; r < r1; r += 4) s += X[(int64_t)r * ld + c];
  red[rg][threadIdx.x & 63] = s;
  __syncthreads();
  if (rg == 0 && c < N) part[(int64_t)blockIdx.y * N + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ void colsum_finish_kernel(const float* __restrict__ part, int nparts, int N, float* out, float* out2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  float t = 0.f;
  for (int p = 0; p < nparts; ++p) t += part[(int64_t)p * N + c];
  out[c] += t;
  if (out2) out2[c] += t;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host
// Each entry point validates, plans (a pure function: no HIP call), makes one scratch request and launches; a small named function
// returns the kernel instance.  The same pattern as gemm_bf16.hip, lstm_resident.hip and misa.hip.
namespace {

bool valid_operands(const mmda_gemm_args& a) {
  return a.A && a.B && a.C && a.M >= 0 && a.N >= 0 && a.K >= 0 && a.batch >= 0 && !(a.gather && a.transA);
}
bool empty_problem(const mmda_gemm_args& a) { return a.M == 0 || a.N == 0 || a.batch == 0; }
// the epilogue knows the unparametrised activations only (mmda_gemm_args has no mmda_act_params; the kernels take any other id for the
// identity), and a problem that has outputs needs a k-tile to make them from (plan_gemm divides by the k-tile count)
bool valid_problem(const mmda_gemm_args& a) {
  return valid_operands(a) && (a.mode == MMDA_F32 || a.mode == MMDA_BF16) && !(a.bias_grad && !a.transA) &&
         a.act >= MMDA_ACT_NONE && a.act <= MMDA_ACT_HARDSHRINK && (a.K > 0 || empty_problem(a));
}
bool plain_epilogue(const mmda_gemm_args& a) { return a.act == MMDA_ACT_NONE && a.drop_p <= 0.f && !a.gate; }
int n_eff(const mmda_gemm_args& a) { return a.N + (a.bias_grad ? 1 : 0); }          // + the virtual ones column
int tiles64(const mmda_gemm_args& a) { return ceil_div(n_eff(a), BN) * ceil_div(a.M, BM) * a.batch; }

// Split-K: these GEMMs are small (B=32: a few dozen output tiles) with long reductions (K = T*B for weight gradients, 2048 for the
// FFN, 4H for the projections); one block per tile would leave 250 CUs idle behind a serial k-loop.  `tiles` output tiles of `nk`
// k-tiles each get enough slices to offer `target` workgroups: at least two k-tiles (64 deep) per slice, at most `cap` slices (cap 1:
// the caller may not split -- an epilogue the reduce launch does not know, or tiles enough already), no empty slice.
constexpr int SPLIT_TARGET_64 = 768, SPLIT_TARGET_128 = 512, SPLIT_TARGET_GROUP = 1024;
constexpr int SPLIT_CAP = 64, SPLIT_CAP_GROUP = 32;
constexpr int SPLIT_MAX_TILES = 256;              // mmda_gemm: a problem with more tiles than this fills the chip unsplit
int splitk_size(int tiles, int nk, int target, int cap) {
  const int sk = nk >= 8 ? max(1, min(ceil_div(target, tiles), min(nk / 2, cap))) : 1;
  return splitk_slices(nk, sk);
}

SplitKJob splitk_job(const mmda_gemm_args& a, const float* slab, int ldn, int sk) {
  SplitKJob J = {};
  J.slab = slab; J.C = a.C; J.M = a.M; J.N = a.N; J.ldn = ldn; J.ldc = a.ldc; J.sk = sk; J.batch = a.batch;
  J.strideC = a.strideC; J.strideBias = a.strideBias; J.alpha = a.alpha; J.bias = a.bias; J.bias2 = a.bias2;
  J.bias_grad = a.bias_grad; J.bias_grad2 = a.bias_grad2; J.accumulate = a.accumulate;
  return J;
}

// large aligned bf16 GEMMs -> 128x128 tile kernel with 16-byte staging loads
bool takes_tile128(const mmda_gemm_args& a) {
  const bool aligned = ((a.lda | a.ldb | a.K) & 3) == 0 && (((uintptr_t)a.A | (uintptr_t)a.B) & 15) == 0 &&
                       ((a.strideA | a.strideB) & 3) == 0 && (!a.transA || (a.M & 3) == 0) && (a.transB || (a.N & 3) == 0);
  return a.mode == MMDA_BF16 && plain_epilogue(a) && aligned && !a.A2 && !a.gather && !a.bias_grad && a.M >= 128 && a.N >= 128;
}

enum class GemmClass { Tile64, Tile64Tiny, Tile128 };      // Tile64Tiny: PF = 4 (see gemm_body)
struct GemmPlan { int rc; GemmClass cls; int sk, ldn; dim3 grid; int64_t slab_floats; };

// everything about the launch of one valid, non-empty problem
GemmPlan plan_gemm(const mmda_gemm_args& a) {
  GemmPlan P = {};
  const bool t128 = takes_tile128(a);
  const int nk = ceil_div(a.K, BK);
  P.ldn = t128 ? a.N : n_eff(a);
  const int tx = ceil_div(P.ldn, t128 ? TN : BN), ty = ceil_div(a.M, t128 ? TM : BM), tiles = tx * ty * a.batch;
  const bool may_split = tiles <= SPLIT_MAX_TILES && (t128 || plain_epilogue(a));
  P.sk = splitk_size(tiles, nk, t128 ? SPLIT_TARGET_128 : SPLIT_TARGET_64, may_split ? SPLIT_CAP : 1);
  P.grid = dim3(tx, ty, a.batch * P.sk);
  if (P.grid.y > 65535 || P.grid.z > 65535) { P.rc = MMDA_EINVAL; return P; }
  const bool tiny = ceil_div(nk, P.sk) <= 4 && (int)(P.grid.x * P.grid.y * P.grid.z) <= 1024;
  P.cls = t128 ? GemmClass::Tile128 : (tiny ? GemmClass::Tile64Tiny : GemmClass::Tile64);
  if (P.sk > 1) P.slab_floats = (int64_t)((size_t)a.batch * P.sk * a.M * P.ldn);
  return P;
}

// (the instances are named in the order the object file has always had them, the 128-tile ones first: DESIGN.md §7)
typedef void (*GemmKernel)(mmda_gemm_args, int, float*, int);
GemmKernel pick_tile128(bool ta, bool tb) {
  if (!ta) return tb ? gemm128_bf16_kernel<false, true> : gemm128_bf16_kernel<false, false>;
  return !tb ? gemm128_bf16_kernel<true, false> : gemm128_bf16_kernel<true, true>;
}
GemmKernel pick_tile64(int mode, bool tiny) {
  if (mode == MMDA_BF16) return tiny ? gemm_kernel<MMDA_BF16, 4> : gemm_kernel<MMDA_BF16, 1>;
  return tiny ? gemm_kernel<MMDA_F32, 4> : gemm_kernel<MMDA_F32, 1>;
}
GemmKernel pick_kernel(GemmClass c, const mmda_gemm_args& a) {
  return c == GemmClass::Tile128 ? pick_tile128(a.transA, a.transB) : pick_tile64(a.mode, c == GemmClass::Tile64Tiny);
}

// One grouped launch.  Slot k runs problem `problem` of the launch's list (the empty ones get no slot) on blocks [start, start + tx *
// ty * batch * sk); slab_off: where its split-K slab starts in the launch's scratch request, in floats (sk > 1 only).
struct GroupSlot { int problem, tx, ty, sk, ldn, start; int64_t slab_off; };
struct GroupPlan { int rc, n, blocks; int64_t slab_floats; GroupSlot slot[GROUP_MAX]; };

// Split-K is sized so that the whole group offers ~4 workgroups per CU; the `absent` problems count into the group without being run.
GroupPlan plan_group(const mmda_gemm_args* args, int cnt, const mmda_gemm_args* absent, int n_absent) {
  GroupPlan P = {};
  int tiles_total = 0;
  for (int i = 0; i < n_absent; ++i) tiles_total += tiles64(absent[i]);
  for (int i = 0; i < cnt; ++i) {
    if (!valid_problem(args[i])) { P.rc = MMDA_EINVAL; return P; }
    tiles_total += tiles64(args[i]);
  }
  for (int i = 0; i < cnt; ++i) {
    const mmda_gemm_args& a = args[i];
    if (empty_problem(a)) continue;
    GroupSlot& S = P.slot[P.n++];
    S.problem = i;
    S.ldn = n_eff(a);
    S.tx = ceil_div(S.ldn, BN); S.ty = ceil_div(a.M, BM);
    S.sk = splitk_size(tiles_total, ceil_div(a.K, BK), SPLIT_TARGET_GROUP,
                       plain_epilogue(a) && tiles_total < SPLIT_TARGET_GROUP ? SPLIT_CAP_GROUP : 1);
    if (S.sk > 1) { S.slab_off = P.slab_floats; P.slab_floats += (int64_t)a.batch * S.sk * a.M * S.ldn; }
    S.start = P.blocks;
    P.blocks += S.tx * S.ty * a.batch * S.sk;
  }
  return P;
}

}  // namespace

extern "C" int mmda_gemm(const mmda_gemm_args* a, void* stream) {
  if (!a || !valid_operands(*a)) return MMDA_EINVAL;
  // An empty problem is MMDA_OK here before its mode, bias_grad and act are looked at; mmda_gemm_grouped rejects a bad one first.  The
  // two orders cannot be made one without changing a return code, so each entry point keeps its own.  (K <= 0 is an error of a
  // problem that has outputs only, in both.)
  if (empty_problem(*a)) return MMDA_OK;
  if (!valid_problem(*a)) return MMDA_EINVAL;
  const GemmPlan P = plan_gemm(*a);
  if (P.rc) return P.rc;
  hipStream_t s = (hipStream_t)stream;
  float* slab = nullptr;
  if (P.sk > 1) {
    slab = mmda_scratch_get(s, sizeof(float) * (size_t)P.slab_floats);
    if (!slab) return MMDA_ELAUNCH;
  }
  hipLaunchKernelGGL(pick_kernel(P.cls, *a), P.grid, dim3(256), 0, s, *a, P.sk, slab, P.ldn);
  MMDA_CHECK_LAUNCH(P.cls == GemmClass::Tile128 ? "mmda_gemm(128)" : "mmda_gemm");
  if (P.sk > 1) { const SplitKJob J = splitk_job(*a, slab, P.ldn, P.sk); return mmda_splitk_reduce(&J, 1, s); }
  return MMDA_OK;
}

extern "C" int mmda_gemm_grouped(const mmda_gemm_args* args, int n, void* stream) {
  return mmda_gemm_grouped_sized(args, n, nullptr, 0, stream);
}

// internal (misa_pass.h): the same launch with its split-K sized as if the `absent` problems were part of it too (they are not run).
// A step that leaves a product out (frozen embedding table: no text layer-1 dX) keeps the slices, and so the bits, of the products
// that stay.  Counted into the first GROUP_MAX problems' launch.
int mmda_gemm_grouped_sized(const mmda_gemm_args* args, int n, const mmda_gemm_args* absent, int n_absent, void* stream) {
  if (!args || n < 0 || n_absent < 0 || (n_absent && !absent)) return MMDA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  for (int base = 0; base < n; base += GROUP_MAX) {
    const GroupPlan P = plan_group(args + base, (n - base) < GROUP_MAX ? (n - base) : GROUP_MAX, absent, base == 0 ? n_absent : 0);
    if (P.rc) return P.rc;
    if (P.blocks == 0) continue;
    float* slab = nullptr;
    if (P.slab_floats) {
      slab = mmda_scratch_get(s, sizeof(float) * (size_t)P.slab_floats);
      if (!slab) return MMDA_ELAUNCH;
    }
    GroupLaunch G;
    SplitKJob jobs[GROUP_MAX];
    int njobs = 0;
    G.n = P.n;
    for (int k = 0; k < P.n; ++k) {
      const GroupSlot& S = P.slot[k];
      G.p[k] = args[base + S.problem];
      G.start[k] = S.start; G.tx[k] = S.tx; G.ty[k] = S.ty; G.splitk[k] = S.sk; G.ldn[k] = S.ldn;
      G.slab[k] = S.sk > 1 ? slab + S.slab_off : nullptr;
      if (S.sk > 1) jobs[njobs++] = splitk_job(G.p[k], G.slab[k], S.ldn, S.sk);
    }
    for (int k = P.n; k <= GROUP_MAX; ++k) G.start[k] = P.blocks;
    for (int k = P.n; k < GROUP_MAX; ++k) { G.p[k] = G.p[0]; G.tx[k] = G.ty[k] = G.splitk[k] = 1; G.slab[k] = nullptr; G.ldn[k] = 0; }
    hipLaunchKernelGGL(gemm_grouped_kernel, dim3(P.blocks), dim3(256), 0, s, G);
    MMDA_CHECK_LAUNCH("mmda_gemm_grouped");
    if (njobs) { const int rc = mmda_splitk_reduce(jobs, njobs, s); if (rc) return rc; }
  }
  return MMDA_OK;
}

// The plans above as a table, one row per input problem: for tests and tools that need to know which instance a shape runs on.  The
// same plan_gemm / plan_group as the launchers; the slab is taken to start 16-byte aligned (the scratch buffer is a hipMalloc
// allocation), so a slot's slab is as aligned as its offset.
extern "C" int mmda_gemm_plan_describe(const mmda_gemm_args* args, int n, int grouped, mmda_gemm_plan_row* rows, int capacity) {
  if (!args || !rows || n < 0 || capacity < n) return MMDA_EINVAL;
  const mmda_gemm_plan_row none = {MMDA_GEMM_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0, 0};
  auto row_of = [&](const mmda_gemm_args& a, int cls, int tx, int ty, int sk, int ldn, int launch, int64_t slab_off) {
    const int nk = ceil_div(a.K, BK), per = ceil_div(nk, sk);
    mmda_gemm_plan_row r = {cls, a.mode, a.transA ? 1 : 0, a.transB ? 1 : 0, tx, ty, sk, per, nk - (sk - 1) * per, ldn,
                            tx * ty * a.batch * sk, launch, slab_off, 0};
    if (sk > 1) {
      const SplitKJob J = splitk_job(a, reinterpret_cast<const float*>((uintptr_t)slab_off * sizeof(float)), ldn, sk);
      r.reduce = splitk_reduce_is_vec(J) ? 2 : 1;
    }
    return r;
  };
  int launches = 0;
  if (!grouped) {
    for (int i = 0; i < n; ++i) {
      const mmda_gemm_args& a = args[i];
      if (!valid_operands(a)) return MMDA_EINVAL;
      rows[i] = none;
      if (empty_problem(a)) continue;
      if (!valid_problem(a)) return MMDA_EINVAL;
      const GemmPlan P = plan_gemm(a);
      if (P.rc) return P.rc;
      static_assert((int)GemmClass::Tile64 == MMDA_GEMM_TILE64 && (int)GemmClass::Tile64Tiny == MMDA_GEMM_TILE64TINY &&
                    (int)GemmClass::Tile128 == MMDA_GEMM_TILE128, "");
      rows[i] = row_of(a, (int)P.cls, (int)P.grid.x, (int)P.grid.y, P.sk, P.ldn, launches++, 0);
    }
    return launches;
  }
  for (int base = 0; base < n; base += GROUP_MAX) {
    const int cnt = (n - base) < GROUP_MAX ? (n - base) : GROUP_MAX;
    const GroupPlan P = plan_group(args + base, cnt, nullptr, 0);
    if (P.rc) return P.rc;
    for (int i = 0; i < cnt; ++i) rows[base + i] = none;
    if (P.blocks == 0) continue;
    for (int k = 0; k < P.n; ++k) {
      const GroupSlot& S = P.slot[k];
      rows[base + S.problem] = row_of(args[base + S.problem], MMDA_GEMM_GROUPSLOT, S.tx, S.ty, S.sk, S.ldn, launches, S.slab_off);
    }
    ++launches;
  }
  return launches;
}

extern "C" int mmda_colsum(const float* X, int ld, int M, int N, float* out, float* out2, void* stream) {
  if (!X || !out || M < 0 || N <= 0) return MMDA_EINVAL;
  if (M == 0) return MMDA_OK;
  int rpb = 256;
  dim3 grid(ceil_div(N, 64), ceil_div(M, rpb));
  float* part = mmda_scratch_get((hipStream_t)stream, sizeof(float) * (size_t)grid.y * N);
  if (!part) return MMDA_ELAUNCH;
  hipLaunchKernelGGL(colsum_kernel, grid, dim3(256), 0, (hipStream_t)stream, X, ld, M, N, part, rpb);
  hipLaunchKernelGGL(colsum_finish_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, part, (int)grid.y, N, out, out2);
  MMDA_CHECK_LAUNCH("mmda_colsum");
  return MMDA_OK;
}
