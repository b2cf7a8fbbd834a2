// Ranking metrics on the device (mmda_amd/ranking.py: ranking_metrics, failure_prediction): how well a score table
// ranks, before any cut-off is chosen.  Three entry points and the plan of the first:
//   mmda_rank_counts           per element (i, c), among the rows j of class c: positives / negatives with s_j > s_i and with s_j == s_i
//   mmda_rank_finish           per class AUROC, AP, AP of the negatives under the negated score and FPR at a TPR level, then their means
//   mmda_rank_rows_accumulate  per row the label-ranking terms (LRAP, ranking loss, coverage) as integers, batch by batch
//   mmda_rank_plan_describe    the launch mmda_rank_counts gives a shape (host only; the launcher reads the same function)
// Scores are compared through one monotone uint32 key (rank_key), so "greater" and "equal" are integer compares and the special values
// are settled once: -0 == +0, a NaN counts as -inf.  Everything counted is an integer (32-bit adds into counts, 64-bit into the row
// state), so no result depends on the order of arrival; the only floating-point sums, the two AP sums of mmda_rank_finish, are
// thread-strided partials added by a fixed tree.  No floating-point atomic anywhere.
#include "internal.h"
#include "eval_terms.h"

namespace {

constexpr int RANK_ROWS = 128;                // elements i per workgroup, one thread each
constexpr int RANK_TILE = 512;                // rows j staged at a time: two lists of at most RANK_TILE keys, 4 KB of LDS
constexpr int RANK_TARGET_WGS = 1024;         // the j rows are split until the grid has about this many workgroups (4 per CU)
constexpr int RANK_FINISH_THREADS = 1024;     // of the one workgroup a class gets in mmda_rank_finish: sixteen waves hide its loads
constexpr int64_t RANK_MAXN = (int64_t)1 << 20;
constexpr int64_t RANK_MAXPAIRS = (int64_t)1 << 42;

// fp32 -> uint32, strictly monotone on the order above: a < b <=> key(a) < key(b), a == b <=> key(a) == key(b).
// NaN -> the bits of -inf, -0 -> +0, then the usual sign flip (negatives inverted, the others get the top bit).
__device__ __forceinline__ unsigned rank_key(float s) {
  unsigned u = __float_as_uint(s);
  if ((u & 0x7fffffffu) > 0x7f800000u) u = 0xff800000u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// keys of list[0 .. n) greater than / equal to ki.  Every lane reads the same address (an LDS broadcast), four keys per read; the
// loop is bounded by n, not padded: no key is "neither greater than nor equal to" the lowest one, which is what a NaN row holds.
__device__ __forceinline__ void rank_count_list(const unsigned* list, int n, unsigned ki, unsigned& g, unsigned& e) {
  int j = 0;
#pragma unroll 2
  for (; j + 4 <= n; j += 4) {
    const uint4 k = *reinterpret_cast<const uint4*>(list + j);
    g += (k.x > ki ? 1u : 0u) + (k.y > ki ? 1u : 0u) + (k.z > ki ? 1u : 0u) + (k.w > ki ? 1u : 0u);
    e += (k.x == ki ? 1u : 0u) + (k.y == ki ? 1u : 0u) + (k.z == ki ? 1u : 0u) + (k.w == ki ? 1u : 0u);
  }
  for (; j < n; ++j) {
    const unsigned k = list[j];
    g += k > ki ? 1u : 0u;
    e += k == ki ? 1u : 0u;
  }
}

// blockIdx.x: RANK_ROWS elements i of class blockIdx.y, one thread each; blockIdx.z: a range of tiles_per_split tiles of the j rows.
// A tile is staged as two compacted key lists (positives, negatives; a wave's places come from one ballot and one LDS add per list,
// and the order inside a list does not matter to a count), so the inner loop is two compares and two adds per pair.
// add == 0: the one split stores its counts; add == 1: counts was cleared in front of the launch and every split adds its share.
__global__ __launch_bounds__(RANK_ROWS) void rank_counts_kernel(const float* __restrict__ scores, const float* __restrict__ truth, int N,
                                                                int C, int tiles_per_split, int add, uint32_t* __restrict__ counts) {
  __shared__ __align__(16) unsigned pos_s[RANK_TILE];
  __shared__ __align__(16) unsigned neg_s[RANK_TILE];
  __shared__ int n_s[2];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int c = blockIdx.y;
  const int i = blockIdx.x * RANK_ROWS + tid;
  const bool live = i < N;
  const unsigned ki = live ? rank_key(scores[(int64_t)i * C + c]) : 0u;
  unsigned gp = 0, gn = 0, ep = 0, en = 0;
  const int64_t jbeg = (int64_t)blockIdx.z * tiles_per_split * RANK_TILE;
  const int64_t jend = jbeg + (int64_t)tiles_per_split * RANK_TILE < N ? jbeg + (int64_t)tiles_per_split * RANK_TILE : N;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t j0 = jbeg; j0 < jend; j0 += RANK_TILE) {
    const int n = (int)(jend - j0 < RANK_TILE ? jend - j0 : RANK_TILE);
    __syncthreads();                                            // the lists of the tile before are read to the end
    if (tid < 2) n_s[tid] = 0;
    __syncthreads();
    for (int k0 = 0; k0 < n; k0 += RANK_ROWS) {
      const int k = k0 + tid;
      if (k - lane >= n) break;                                 // the whole wave is past the tile
      const bool in = k < n;
      unsigned key = 0u;
      bool p = false;
      if (in) {
        const int64_t el = (j0 + k) * C + c;
        key = rank_key(scores[el]);
        p = truth[el] > 0.f;
      }
      const unsigned long long mp = __ballot(in && p), mq = __ballot(in && !p);
      int bp = 0, bq = 0;
      if (lane == 0) {
        bp = atomicAdd(&n_s[0], __popcll(mp));
        bq = atomicAdd(&n_s[1], __popcll(mq));
      }
      bp = __shfl(bp, 0);
      bq = __shfl(bq, 0);
      if (in) {
        if (p) pos_s[bp + __popcll(mp & below)] = key;          // bp + its place < n_s[0] <= n <= RANK_TILE
        else neg_s[bq + __popcll(mq & below)] = key;
      }
    }
    __syncthreads();
    rank_count_list(pos_s, n_s[0], ki, gp, ep);
    rank_count_list(neg_s, n_s[1], ki, gn, en);
  }
  if (!live) return;
  uint32_t* out = counts + ((int64_t)i * C + c) * 4;
  if (!add) {
    *reinterpret_cast<uint4*>(out) = make_uint4(gp, gn, ep, en);
  } else {
    if (gp) atomicAdd(out + 0, gp);
    if (gn) atomicAdd(out + 1, gn);
    if (ep) atomicAdd(out + 2, ep);
    if (en) atomicAdd(out + 3, en);
  }
}

// ------------------------------------------------------------------------------------------------ finish
// One workgroup of RANK_FINISH_THREADS threads per class, elements thread-strided.  Pass 1 counts the positives (the FPR's `need`
// depends on them), pass 2 makes the four reductions.  A reduction is the xor butterfly inside a wave (the same bits in every lane:
// each step combines the same two numbers on both sides), then the wave results in wave order: a fixed tree for the fp64 sums.
__global__ __launch_bounds__(RANK_FINISH_THREADS) void rank_finish_kernel(const uint32_t* __restrict__ counts,
                                                                          const float* __restrict__ truth, int N, int C, double level,
                                                                          double* __restrict__ out) {
  constexpr int WAVES = RANK_FINISH_THREADS / WAVE;
  __shared__ unsigned long long p_s[WAVES], num_s[WAVES], min_s[WAVES];
  __shared__ double ap_s[WAVES], apn_s[WAVES];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  unsigned long long P = 0;
  for (int i = tid; i < N; i += RANK_FINISH_THREADS) P += truth[(int64_t)i * C + c] > 0.f ? 1ull : 0ull;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) P += __shfl_xor(P, o);
  if (lane == 0) p_s[wave] = P;
  __syncthreads();
  P = 0;
  for (int w = 0; w < WAVES; ++w) P += p_s[w];                             // every thread needs it
  const unsigned long long Nn = (unsigned long long)N - P;
  RankFigures<WAVES> fig(level, P);
  for (int i = tid; i < N; i += RANK_FINISH_THREADS) {
    const int64_t el = (int64_t)i * C + c;
    const uint4 k = *reinterpret_cast<const uint4*>(counts + el * 4);      // gp, gn, ep, en
    const unsigned long long gp = k.x, gn = k.y, ep = k.z, en = k.w;
    if (truth[el] > 0.f) fig.positive(1ull, gp + ep, gn, gn + en, Nn);     // ep >= 1: the element itself
    else fig.negative(1ull, gp, gn, P, Nn);                               // en >= 1
  }
  if (fig.reduce(num_s, min_s, ap_s, apn_s)) fig.write(P, Nn, out + (int64_t)c * 6);
}

// Row C of the table, by one thread behind the class rows.
__global__ void rank_macro_kernel(int C, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) rank_macro_row(C, out);
}

// ------------------------------------------------------------------------------------------------ label ranking, per row
// One thread per row: its C keys in registers, every positive j against every k.  The row's terms are integers (rank_j <= 16 divides
// EVAL_LCM), added per workgroup in LDS (64-bit) and from there, where non-zero, into the state.
__global__ __launch_bounds__(256) void rank_rows_kernel(const float* __restrict__ scores, const float* __restrict__ truth, int64_t N, int C,
                                                        unsigned long long* __restrict__ state) {
  __shared__ unsigned long long acc_s[2 + 3 * (EVAL_MAXC + 1)];
  const int words = 2 + 3 * (C + 1);
  for (int w = threadIdx.x; w < words; w += 256) acc_s[w] = 0ull;
  __syncthreads();
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < N; row += (int64_t)gridDim.x * 256) {
    unsigned key[EVAL_MAXC];
    unsigned posmask = 0u;
#pragma unroll
    for (int c = 0; c < EVAL_MAXC; ++c) {
      key[c] = 0u;
      if (c < C) {
        key[c] = rank_key(scores[row * C + c]);
        posmask |= (truth[row * C + c] > 0.f ? 1u : 0u) << c;
      }
    }
    unsigned lrap = 0u, bad = 0u, cov = 0u;
#pragma unroll
    for (int j = 0; j < EVAL_MAXC; ++j) {
      if (j < C && ((posmask >> j) & 1u)) {
        unsigned rank = 0u, L = 0u;
#pragma unroll
        for (int k = 0; k < EVAL_MAXC; ++k) {
          if (k < C) {
            const unsigned ge = key[k] >= key[j] ? 1u : 0u;
            rank += ge;
            L += ge & (posmask >> k);
          }
        }
        lrap += L * ((unsigned)EVAL_LCM / rank);                          // rank >= 1: k == j
        bad += rank - L;
        cov = rank > cov ? rank : cov;
      }
    }
    const int P = __popc(posmask);
    atomicAdd(&acc_s[0], 1ull);
    if (cov) atomicAdd(&acc_s[1], (unsigned long long)cov);
    atomicAdd(&acc_s[2 + P], 1ull);
    if (lrap) atomicAdd(&acc_s[2 + (C + 1) + P], (unsigned long long)lrap);
    if (bad) atomicAdd(&acc_s[2 + 2 * (C + 1) + P], (unsigned long long)bad);
  }
  __syncthreads();
  for (int w = threadIdx.x; w < words; w += 256) {
    const unsigned long long v = acc_s[w];
    if (v) atomicAdd(&state[w], v);
  }
}

// what the three entry points accept for (N, C)
bool rank_shape_ok(int64_t N, int C) {
  return C >= 1 && C <= EVAL_MAXC && N >= 0 && N <= RANK_MAXN && N * N * C <= RANK_MAXPAIRS;
}

}  // namespace

extern "C" int mmda_rank_plan_describe(int64_t N, int C, mmda_rank_plan* out) {
  if (!out || !rank_shape_ok(N, C)) return MMDA_EINVAL;
  mmda_rank_plan p{};
  p.rows_per_wg = RANK_ROWS;
  p.tile = RANK_TILE;
  p.tiles = (int)ceil_div64(N, RANK_TILE);
  p.grid_x = (int)ceil_div64(N, RANK_ROWS);
  p.grid_y = C;
  p.counts_bytes = N * C * 4 * (int64_t)sizeof(uint32_t);
  if (N > 0) {
    // few row blocks: split the j rows until the launch has workgroups to spread over; never an empty split
    int want = ceil_div(RANK_TARGET_WGS, p.grid_x * C);
    if (want > p.tiles) want = p.tiles;
    p.tiles_per_split = ceil_div(p.tiles, want);
    p.splits = ceil_div(p.tiles, p.tiles_per_split);
  }
  p.grid_z = p.splits;
  *out = p;
  return MMDA_OK;
}

extern "C" int mmda_rank_counts(const float* scores, const float* truth, int64_t N, int C, uint32_t* counts, void* stream) {
  if (!scores || !truth || !counts || ((uintptr_t)counts & 15)) return MMDA_EINVAL;
  mmda_rank_plan p;
  if (mmda_rank_plan_describe(N, C, &p) != MMDA_OK) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  if (p.splits > 1) {
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)p.counts_bytes, (hipStream_t)stream);
    if (e != hipSuccess) { mmda_set_error("mmda_rank_counts", e); return MMDA_ELAUNCH; }
  }
  hipLaunchKernelGGL(rank_counts_kernel, dim3(p.grid_x, p.grid_y, p.grid_z), dim3(RANK_ROWS), 0, (hipStream_t)stream, scores, truth, (int)N,
                     C, p.tiles_per_split, p.splits > 1 ? 1 : 0, counts);
  MMDA_CHECK_LAUNCH("mmda_rank_counts");
  return MMDA_OK;
}

extern "C" int mmda_rank_finish(const uint32_t* counts, const float* truth, int64_t N, int C, double tpr_level, double* out, void* stream) {
  if (!counts || !truth || !out || ((uintptr_t)counts & 15) || ((uintptr_t)out & 7)) return MMDA_EINVAL;
  if (!rank_shape_ok(N, C) || !(tpr_level > 0.0 && tpr_level <= 1.0)) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  hipLaunchKernelGGL(rank_finish_kernel, dim3(C), dim3(RANK_FINISH_THREADS), 0, (hipStream_t)stream, counts, truth, (int)N, C, tpr_level, out);
  MMDA_CHECK_LAUNCH("mmda_rank_finish");
  hipLaunchKernelGGL(rank_macro_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, C, out);
  MMDA_CHECK_LAUNCH("mmda_rank_finish");
  return MMDA_OK;
}

extern "C" int mmda_rank_rows_accumulate(const float* scores, const float* truth, int64_t N, int C, unsigned long long* state,
                                         void* stream) {
  if (!scores || !truth || !state || ((uintptr_t)state & 7)) return MMDA_EINVAL;
  if (!rank_shape_ok(N, C)) return MMDA_EINVAL;
  if (N == 0) return MMDA_OK;
  const int blocks = (int)(ceil_div64(N, 256) < 256 ? ceil_div64(N, 256) : 256);
  hipLaunchKernelGGL(rank_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, scores, truth, N, C, state);
  MMDA_CHECK_LAUNCH("mmda_rank_rows_accumulate");
  return MMDA_OK;
}
