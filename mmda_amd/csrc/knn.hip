// Exact set-wise k-nearest-neighbour search between two device tables, and the Trust Score table built on it (mmda_amd/neighbours.py,
// DESIGN.md 4t).  Entry points:
//   mmda_knn_plan_describe  the launches of a shape: query tile, slabs, grid, LDS and work bytes (host only; the launcher reads it)
//   mmda_knn_sets           per (query row, set) the k nearest member rows of the base: (Q, S, k) squared distances and row numbers
//   mmda_trust_score        (n, 2 C, k) distances + decisions -> the (n, C) float64 ratio other / predicted
// The search is three launches.  Row norms first.  Then grid (query tiles, slabs): a workgroup walks its slab of the base in tiles of
// 128 rows, forms the TQ x 128 products q.b on the f32-input MFMA from operands staged through LDS, turns them into
// |q|^2 + |b|^2 - 2 q.b in LDS and lets each wave update the running lists of its query rows from that tile -- the Q x N matrix never
// reaches memory.  The last launch merges the slabs' lists, recomputes the k survivors as sum (q_i - b_i)^2 and sorts them again.
//
// Order and ties.  Everything is ordered by (distance, row number).  A workgroup meets the rows of its slab in ascending order, so a
// candidate enters a list only when it is STRICTLY nearer than the list's last entry and goes behind every entry that is not farther:
// equal distances stay in row order without the row number being compared.  The merge and the final sort compare both.
//
// Bits.  The product of a pair is one fmaf chain over i = 0 .. D - 1 from 0 (what v_mfma_f32_32x32x2_f32 computes; the zero padding
// of D to a multiple of 32 adds fmaf(0, 0, c) = c), the norms and the direct form are sums whose order is a function of D alone, so
// the distance of a pair depends on the two rows and D only: not on the tile, the slab, Q or the run.  No float atomics.
#include "internal.h"
#include "dynamic_lds.h"

// every product that is fused into a sum is written as fmaf; nothing else may be
#pragma clang fp contract(off)

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int KNN_TB = 128;                    // base rows of one distance tile
constexpr int KNN_KC = 32;                     // elements of D staged per piece
constexpr int KNN_PITCH = KNN_KC + 1;          // of a staged row, in floats: the MFMA operand reads walk rows
constexpr int KNN_THREADS = 256;
constexpr int KNN_MAXD = 1024, KNN_MAXS = 16, KNN_MAXK = 16;
constexpr int KNN_MAX_SLABS = 32;              // the merge holds slabs * k <= 512 candidates, 8 per lane
constexpr int KNN_TARGET_WGS = 256;            // one workgroup per CU of an MI355X: the lists leave room for one
constexpr int KNN_WIDE_LISTS = 200;            // S k up to here: 64 query rows per workgroup, above: 32
constexpr int64_t KNN_PART_ROWS = 16384;       // slabs * Q never exceeds max(Q, this): slabs * ceil(Q / tile_q) <= KNN_TARGET_WGS
constexpr int KNN_LDS_LIMIT = 160 * 1024;

struct KnnArgs {
  const float* query; const float* base; const uint32_t* member;
  float* qn; float* bn; float* part_d; int32_t* part_i;
  int64_t Q, N, slab_rows;
  int D, S, k, exclude_self;
};

__host__ __device__ constexpr int knn_lds_floats(int tq, int S, int k) {
  return (tq + KNN_TB) * KNN_PITCH + tq * KNN_TB + tq + 2 * KNN_TB + 2 * tq * S * k;
}

__device__ __forceinline__ float knn_inf() { return __builtin_huge_valf(); }

// lane l adds the elements l, l + 64, ... in that order, a fixed xor butterfly adds the lanes: every lane returns the same bits
__device__ __forceinline__ float knn_lanes_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float knn_direct(const float* __restrict__ q, const float* __restrict__ b, int D, int lane) {
  float acc = 0.f;
  for (int i = lane; i < D; i += WAVE) { const float t = q[i] - b[i]; acc = fmaf(t, t, acc); }
  return knn_lanes_sum(acc);
}

// ------------------------------------------------------------------------------------------------ launch 1: row norms
__global__ __launch_bounds__(KNN_THREADS) void knn_norms_kernel(KnnArgs a) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int64_t rows = a.Q + a.N;
  for (int64_t r = (int64_t)blockIdx.x * (KNN_THREADS / WAVE) + wave; r < rows; r += (int64_t)gridDim.x * (KNN_THREADS / WAVE)) {
    const float* x = r < a.Q ? a.query + r * a.D : a.base + (r - a.Q) * a.D;
    float acc = 0.f;
    for (int i = lane; i < a.D; i += WAVE) acc = fmaf(x[i], x[i], acc);
    acc = knn_lanes_sum(acc);
    if (lane == 0) { if (r < a.Q) a.qn[r] = acc; else a.bn[r - a.Q] = acc; }
  }
}

// ------------------------------------------------------------------------------------------------ launch 2: tiles and lists
template <bool VEC>
__device__ __forceinline__ float4 knn_load4(const float* __restrict__ row, int i, int D) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row == nullptr) return v;
  if (VEC) {
    if (i < D) v = *reinterpret_cast<const float4*>(row + i);           // D % 4 == 0: i + 3 < D
  } else {
    if (i < D) v.x = row[i];
    if (i + 1 < D) v.y = row[i + 1];
    if (i + 2 < D) v.z = row[i + 2];
    if (i + 3 < D) v.w = row[i + 3];
  }
  return v;
}

// The candidate (cd, ci) -- wave-uniform, its row number above every row the list holds -- enters the list the lanes 0 .. k - 1 hold
// (ascending; lanes from k on hold +inf) when it is strictly nearer than the last entry: behind every entry that is not farther.
__device__ __forceinline__ void knn_insert(float& e_d, int& e_i, float cd, int ci, int k, int lane) {
  const float last = __shfl(e_d, k - 1);
  if (cd < last) {
    const int pos = __popcll(__ballot(lane < k && e_d <= cd));            // < k
    const float pd = __shfl_up(e_d, 1);
    const int pi = __shfl_up(e_i, 1);
    if (lane > pos) { e_d = pd; e_i = pi; }
    else if (lane == pos) { e_d = cd; e_i = ci; }
  }
}

// grid (query tiles, slabs), 4 waves.  Wave w forms columns 32 w .. 32 w + 31 of the TQ x 128 tile (TQ / 32 accumulators of 32 x 32),
// then owns the lists of the query rows w TQ / 4 .. : per row the 128 distances sit two to a lane, and per set a ballot says whether
// any of them beats the list's last entry; only then is the list (k entries, lanes 0 .. k - 1) read, updated by shuffles and written.
template <int TQ, bool VEC>
__global__ __launch_bounds__(KNN_THREADS) void knn_tiles_kernel(KnnArgs a) {
  extern __shared__ float knn_lds[];
  constexpr int RB = TQ / 32;                   // accumulators per wave
  float* Qs = knn_lds;                          // [TQ][PITCH]
  float* Bs = Qs + TQ * KNN_PITCH;              // [128][PITCH]
  float* distS = Bs + KNN_TB * KNN_PITCH;       // [TQ][128]
  float* qnS = distS + TQ * KNN_TB;             // [TQ]
  float* bnS = qnS + TQ;                        // [128]
  uint32_t* memS = reinterpret_cast<uint32_t*>(bnS + KNN_TB);      // [128]
  float* ld = bnS + 2 * KNN_TB;                 // [TQ][S][k]
  int* li = reinterpret_cast<int*>(ld + TQ * a.S * a.k);

  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int D = a.D, S = a.S, k = a.k;
  const int64_t q0 = (int64_t)blockIdx.x * TQ;
  const int64_t slab0 = (int64_t)blockIdx.y * a.slab_rows;
  const int64_t slab1 = slab0 + a.slab_rows < a.N ? slab0 + a.slab_rows : a.N;
  const int entries = TQ * S * k;
  for (int e = tid; e < entries; e += KNN_THREADS) { ld[e] = knn_inf(); li[e] = -1; }
  for (int r = tid; r < TQ; r += KNN_THREADS) qnS[r] = q0 + r < a.Q ? a.qn[q0 + r] : 0.f;

  const int k4 = (tid & 7) * 4, srow = tid >> 3;      // staging: 8 threads along a row's 32 floats, 32 rows per sweep
  const int pieces = (D + KNN_KC - 1) / KNN_KC;
  const int mrow = lane & 31, mh = lane >> 5;         // MFMA operand: row / column mrow, element mh of the pair

  for (int64_t b0 = slab0; b0 < slab1; b0 += KNN_TB) {
    float4 rq[RB], rb[KNN_TB / 32];
    auto fetch = [&](int piece) {
      const int i = piece * KNN_KC + k4;
#pragma unroll
      for (int u = 0; u < RB; ++u) {
        const int64_t g = q0 + srow + 32 * u;
        rq[u] = knn_load4<VEC>(g < a.Q ? a.query + g * D : nullptr, i, D);
      }
#pragma unroll
      for (int u = 0; u < KNN_TB / 32; ++u) {
        const int64_t g = b0 + srow + 32 * u;
        rb[u] = knn_load4<VEC>(g < a.N ? a.base + g * D : nullptr, i, D);
      }
    };
    f32x16 acc[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[u][e] = 0.f;
    fetch(0);
    for (int piece = 0; piece < pieces; ++piece) {
      __syncthreads();                          // the last piece's operands are read; on piece 0: the last tile's lists are done
      if (piece == 0 && tid < KNN_TB) {
        const int64_t g = b0 + tid;
        bnS[tid] = g < a.N ? a.bn[g] : 0.f;
        memS[tid] = g < a.N ? a.member[g] : 0u;
      }
#pragma unroll
      for (int u = 0; u < RB; ++u) {
        float* dst = Qs + (srow + 32 * u) * KNN_PITCH + k4;
        dst[0] = rq[u].x; dst[1] = rq[u].y; dst[2] = rq[u].z; dst[3] = rq[u].w;
      }
#pragma unroll
      for (int u = 0; u < KNN_TB / 32; ++u) {
        float* dst = Bs + (srow + 32 * u) * KNN_PITCH + k4;
        dst[0] = rb[u].x; dst[1] = rb[u].y; dst[2] = rb[u].z; dst[3] = rb[u].w;
      }
      __syncthreads();
      if (piece + 1 < pieces) fetch(piece + 1);  // in flight under the MFMAs
      const float* bp = Bs + (wave * 32 + mrow) * KNN_PITCH + mh;
      const float* ap = Qs + mrow * KNN_PITCH + mh;
#pragma unroll
      for (int kk = 0; kk < KNN_KC / 2; ++kk) {
        const float bv = bp[2 * kk];
#pragma unroll
        for (int u = 0; u < RB; ++u)
          acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[u * 32 * KNN_PITCH + 2 * kk], bv, acc[u], 0, 0, 0);
      }
    }
    // the tile's distances: accumulator register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
    {
      const int col = wave * 32 + mrow;
      const float bnv = bnS[col];
#pragma unroll
      for (int u = 0; u < RB; ++u)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = u * 32 + (e & 3) + 8 * (e >> 2) + 4 * mh;
          distS[row * KNN_TB + col] = fmaf(-2.f, acc[u][e], qnS[row] + bnv);
        }
    }
    __syncthreads();
    uint32_t m0 = memS[lane], m1 = memS[lane + WAVE];
    for (int rr = 0; rr < TQ / 4; ++rr) {
      const int r = wave * (TQ / 4) + rr;
      const int64_t gq = q0 + r;
      if (gq >= a.Q) break;
      const float d0 = distS[r * KNN_TB + lane], d1 = distS[r * KNN_TB + lane + WAVE];
      uint32_t w0 = m0, w1 = m1;
      if (a.exclude_self) {
        if (b0 + lane == gq) w0 = 0u;
        if (b0 + lane + WAVE == gq) w1 = 0u;
      }
      for (int s = 0; s < S; ++s) {
        const int at = (r * S + s) * k;
        const float thr = ld[at + k - 1];
        unsigned long long h0 = __ballot(((w0 >> s) & 1u) && d0 < thr);
        unsigned long long h1 = __ballot(((w1 >> s) & 1u) && d1 < thr);
        if ((h0 | h1) == 0ull) continue;
        float e_d = lane < k ? ld[at + lane] : knn_inf();
        int e_i = lane < k ? li[at + lane] : -1;
        while (h0) {
          const int src = __ffsll((long long)h0) - 1;
          h0 &= h0 - 1ull;
          knn_insert(e_d, e_i, __shfl(d0, src), (int)(b0 + src), k, lane);
        }
        while (h1) {
          const int src = __ffsll((long long)h1) - 1;
          h1 &= h1 - 1ull;
          knn_insert(e_d, e_i, __shfl(d1, src), (int)(b0 + WAVE + src), k, lane);
        }
        if (lane < k) { ld[at + lane] = e_d; li[at + lane] = e_i; }
      }
    }
  }
  __syncthreads();
  const int per_row = S * k;
  for (int e = tid; e < entries; e += KNN_THREADS) {
    const int64_t gq = q0 + e / per_row;
    if (gq < a.Q) {
      const int64_t off = ((int64_t)blockIdx.y * a.Q + gq) * per_row + e % per_row;
      a.part_d[off] = ld[e];
      a.part_i[off] = li[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------ launch 3: merge, refine, sort
// One wave per (query row, set).  The slabs' lists (slabs * k <= 512 candidates, 8 to a lane) give their k least by (distance, row
// number); each survivor's distance is recomputed in the direct form; the survivors are ranked by (that distance, row number).
__global__ __launch_bounds__(KNN_THREADS) void knn_finish_kernel(KnnArgs a, int slabs, float* __restrict__ dist, int32_t* __restrict__ index) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int S = a.S, k = a.k, D = a.D;
  const int64_t pairs = a.Q * S;
  const int total = slabs * k;
  for (int64_t p = (int64_t)blockIdx.x * (KNN_THREADS / WAVE) + wave; p < pairs; p += (int64_t)gridDim.x * (KNN_THREADS / WAVE)) {
    const int64_t q = p / S;
    const int s = (int)(p % S);
    float cd[8];
    unsigned ci[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = lane + WAVE * u;
      cd[u] = knn_inf(); ci[u] = 0xffffffffu;
      if (c < total) {
        const int64_t off = (((int64_t)(c / k) * a.Q + q) * S + s) * k + c % k;
        cd[u] = a.part_d[off]; ci[u] = (unsigned)a.part_i[off];
      }
    }
    float sel_d = knn_inf();
    unsigned sel_i = 0xffffffffu;
    for (int t = 0; t < k; ++t) {
      float bd = knn_inf();
      unsigned bi = 0xffffffffu;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (cd[u] < bd || (cd[u] == bd && ci[u] < bi)) { bd = cd[u]; bi = ci[u]; }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float od = __shfl_xor(bd, o);
        const unsigned oi = (unsigned)__shfl_xor((int)bi, o);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
      }
      if (bi == 0xffffffffu) break;             // uniform: nothing but padding is left
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (ci[u] == bi) { cd[u] = knn_inf(); ci[u] = 0xffffffffu; }
      if (lane == t) { sel_d = bd; sel_i = bi; }
    }
    const float* qrow = a.query + q * D;
    float ref = knn_inf();
    for (int j = 0; j < k; ++j) {
      const int bi = __shfl((int)sel_i, j);
      if (bi < 0) break;                        // uniform: the valid entries are a prefix
      const float v = knn_direct(qrow, a.base + (int64_t)bi * D, D, lane);
      if (lane == j) ref = v;
    }
    (void)sel_d;
    int rank = 0;
    for (int l = 0; l < k; ++l) {
      const float od = __shfl(ref, l);
      const unsigned oi = (unsigned)__shfl((int)sel_i, l);
      rank += (od < ref || (od == ref && (oi < sel_i || (oi == sel_i && l < lane)))) ? 1 : 0;
    }
    if (lane < k) {
      const int64_t off = (q * S + s) * k + rank;
      dist[off] = ref;
      index[off] = (int32_t)sel_i;
    }
  }
}

// ------------------------------------------------------------------------------------------------ the Trust Score table
__global__ __launch_bounds__(256) void trust_score_kernel(const float* __restrict__ dist, const int32_t* __restrict__ index,
                                                          const float* __restrict__ labels, int64_t n, int C, int k,
                                                          double* __restrict__ trust, float* __restrict__ d_pred, float* __restrict__ d_other,
                                                          int32_t* __restrict__ nearest_pred, int32_t* __restrict__ nearest_other) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n * C; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / C;
    const int c = (int)(e % C);
    const int y = labels[e] > 0.f ? 1 : 0;
    const int64_t at_p = ((i * 2 * C) + 2 * c + y) * k, at_o = ((i * 2 * C) + 2 * c + 1 - y) * k;
    const float p = dist[at_p], o = dist[at_o];
    double t;
    if (p == knn_inf()) t = 0.0;
    else t = sqrt((double)o) / (sqrt((double)p) + 1e-12);
    trust[e] = t;
    if (d_pred) d_pred[e] = p;
    if (d_other) d_other[e] = o;
    if (nearest_pred) nearest_pred[e] = index[at_p];
    if (nearest_other) nearest_other[e] = index[at_o];
  }
}

bool knn_shape_ok(int64_t Q, int64_t N, int D, int S, int k) {
  return Q >= 0 && Q <= INT32_MAX && N >= 1 && N <= INT32_MAX && D >= 1 && D <= KNN_MAXD && S >= 1 && S <= KNN_MAXS && k >= 1 && k <= KNN_MAXK;
}

int64_t knn_round4(int64_t n) { return (n + 3) / 4 * 4; }

template <int TQ>
void knn_launch_tiles(const KnnArgs& a, const mmda_knn_plan& p, bool vec, hipStream_t stream) {
  const dim3 grid(p.grid_x, p.grid_y);
  if (vec) {
    ensure_dynamic_lds(knn_tiles_kernel<TQ, true>, (size_t)p.lds_bytes);
    hipLaunchKernelGGL((knn_tiles_kernel<TQ, true>), grid, dim3(KNN_THREADS), (size_t)p.lds_bytes, stream, a);
  } else {
    ensure_dynamic_lds(knn_tiles_kernel<TQ, false>, (size_t)p.lds_bytes);
    hipLaunchKernelGGL((knn_tiles_kernel<TQ, false>), grid, dim3(KNN_THREADS), (size_t)p.lds_bytes, stream, a);
  }
}

}  // namespace

extern "C" int mmda_knn_plan_describe(int64_t Q, int64_t N, int D, int S, int k, mmda_knn_plan* out) {
  if (!out || !knn_shape_ok(Q, N, D, S, k)) return MMDA_EINVAL;
  mmda_knn_plan p{};
  p.tile_q = S * k <= KNN_WIDE_LISTS ? 64 : 32;
  p.tile_b = KNN_TB;
  const int64_t tiles_q = Q > 0 ? ceil_div64(Q, p.tile_q) : 1;
  const int64_t tiles_b = ceil_div64(N, KNN_TB);
  int64_t slabs = KNN_TARGET_WGS / tiles_q;      // as many slabs as keep the grid within one workgroup per CU
  if (slabs > KNN_MAX_SLABS) slabs = KNN_MAX_SLABS;
  if (slabs > tiles_b) slabs = tiles_b;
  if (slabs < 1) slabs = 1;
  const int64_t slab_tiles = ceil_div64(tiles_b, slabs);
  slabs = ceil_div64(tiles_b, slab_tiles);
  p.slab_rows = (int)(slab_tiles * KNN_TB > INT32_MAX ? (int64_t)INT32_MAX / KNN_TB * KNN_TB : slab_tiles * KNN_TB);
  p.slabs = (int)slabs;
  p.merge = slabs > 1;
  p.launches = 3;
  p.grid_x = (int)tiles_q;
  p.grid_y = (int)slabs;
  p.threads = KNN_THREADS;
  p.lds_bytes = (int)sizeof(float) * knn_lds_floats(p.tile_q, S, k);
  p.vector_loads = D % 4 == 0;
  p.max_slabs = KNN_MAX_SLABS;
  // the lists: slabs * Q rows of S k entries, sized by a bound that only grows with Q (slabs falls as Q grows)
  int64_t part_rows = Q * KNN_MAX_SLABS < KNN_PART_ROWS ? Q * KNN_MAX_SLABS : KNN_PART_ROWS;
  if (part_rows < Q) part_rows = Q;
  p.work_bytes = (int64_t)sizeof(float) * (knn_round4(Q) + knn_round4(N)) + 8 * part_rows * S * k;
  if (p.lds_bytes > KNN_LDS_LIMIT) return MMDA_EINVAL;
  *out = p;
  return MMDA_OK;
}

extern "C" int mmda_knn_sets(const float* query, const float* base, const uint32_t* member, int64_t Q, int64_t N, int D, int S, int k,
                             int exclude_self, float* dist, int32_t* index, void* work, int64_t work_bytes, void* stream) {
  if (!query || !base || !member || !dist || !index || !work || ((uintptr_t)work & 15)) return MMDA_EINVAL;
  mmda_knn_plan p;
  if (mmda_knn_plan_describe(Q, N, D, S, k, &p) != MMDA_OK || work_bytes < p.work_bytes) return MMDA_EINVAL;
  if (Q == 0) return MMDA_OK;
  if ((int64_t)p.slabs * Q > (p.work_bytes - (int64_t)sizeof(float) * (knn_round4(Q) + knn_round4(N))) / (8 * S * k)) return MMDA_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  KnnArgs a{};
  a.query = query; a.base = base; a.member = member;
  a.qn = static_cast<float*>(work);
  a.bn = a.qn + knn_round4(Q);
  a.part_d = a.bn + knn_round4(N);
  a.part_i = reinterpret_cast<int32_t*>(a.part_d + (int64_t)p.slabs * Q * S * k);
  a.Q = Q; a.N = N; a.slab_rows = p.slab_rows;
  a.D = D; a.S = S; a.k = k; a.exclude_self = exclude_self != 0;
  hipLaunchKernelGGL(knn_norms_kernel, dim3(stream_blocks((Q + N) * 64)), dim3(KNN_THREADS), 0, st, a);
  MMDA_CHECK_LAUNCH("mmda_knn_sets (norms)");
  const bool vec = p.vector_loads && !(((uintptr_t)query | (uintptr_t)base) & 15);
  if (p.tile_q == 64) knn_launch_tiles<64>(a, p, vec, st); else knn_launch_tiles<32>(a, p, vec, st);
  MMDA_CHECK_LAUNCH("mmda_knn_sets (tiles)");
  hipLaunchKernelGGL(knn_finish_kernel, dim3(stream_blocks(Q * S * 64)), dim3(KNN_THREADS), 0, st, a, p.slabs, dist, index);
  MMDA_CHECK_LAUNCH("mmda_knn_sets (finish)");
  return MMDA_OK;
}

extern "C" int mmda_trust_score(const float* dist, const int32_t* index, const float* labels, int64_t n, int C, int k, double* trust,
                                float* d_pred, float* d_other, int32_t* nearest_pred, int32_t* nearest_other, void* stream) {
  if (!dist || !labels || !trust || n < 0 || C < 1 || C > KNN_MAXS / 2 || k < 1 || k > KNN_MAXK) return MMDA_EINVAL;
  if ((nearest_pred || nearest_other) && !index) return MMDA_EINVAL;
  if (n == 0) return MMDA_OK;
  hipLaunchKernelGGL(trust_score_kernel, dim3(stream_blocks(n * C)), dim3(256), 0, (hipStream_t)stream, dist, index, labels, n, C, k, trust,
                     d_pred, d_other, nearest_pred, nearest_other);
  MMDA_CHECK_LAUNCH("mmda_trust_score");
  return MMDA_OK;
}
