// The rows of the embedding table: the gather, and everything that turns a list of (id, row) pairs into updates of table rows,
// deterministically (one writer per table row, sums in list order, no float atomics).
//   * a ROW RULE says what a row's finished sum does (common.h): RowAdd adds it into the dense gradient, RowSparseAdam and RowDenseAdam
//     update the table and its moments in place (embed_update = sparse / deferred).
//   * a LIST FORM says how the sums are made: SHORT, one workgroup per position that scans the id list (at most ES_MAX positions);
//     SORT, a stable radix sort of the ids and two levels of list-order sums; PRESORTED, the two levels over a list that
//     mmda_embed_sort_ids sorted earlier (a training step sorts beside a recurrence, only the sums wait for the gradient rows).
// One kernel template per form takes the rule by value; one host launcher, embed_rows_apply, checks the list, picks the form
// (list_form, the only place that does), carves the work buffer and launches.  Every entry below is a call of it.  Also here: the
// deferred update's replay kernels (catch-up, flush) and the list that accumulation appends a micro-batch's rows to.
// mmda_embed_segment_sum is the data-parallel entry: ranks exchange the embedding gradient as all-gathered (ids, rows)
// -- at most T*B rows per rank instead of V rows -- and every rank runs it on the same gathered list, in the same order, so the replicas
// stay bit-identical.
#include "common.h"
#include "internal.h"
#include <math.h>
#include <hipcub/hipcub.hpp>

namespace {

// stamp != nullptr: the row of the table a position reads is stamped with the step's epoch on the way (internal.h: RowStamp; st.ids and
// st.n are this launch's own ids and rows)
__global__ void embed_gather_kernel(const float* __restrict__ W, const int64_t* __restrict__ ids, int rows, int dim, float* out,
                                    unsigned* stamp, unsigned epoch, int table_rows) {
  int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (stamp && (threadIdx.x & 63) == 0 && ids[row] >= 0 && ids[row] < table_rows) stamp[ids[row]] = epoch;
  const float* src = W + ids[row] * (int64_t)dim;
  float* dst = out + (int64_t)row * dim;
  for (int i = threadIdx.x & 63; i < dim; i += 64) dst[i] = src[i];
}

// ---- the short form
// dW[ids[p]] += dX[p] for every position p, deterministically: one workgroup per position; the workgroup of the FIRST position that
// holds an id owns that id -- it marks every position with the same id in an LDS bit mask (one pass over the id list), compacts the
// marks into an ordered list, and its four waves add the rows of four contiguous quarters of that list in position order (eight row
// loads in flight per lane and dimension group), the quarters' sums are added in order and the total goes to the table row (single
// writer: no atomics, identical bits on every run; float atomics gave the rows of repeated ids in arrival order).  Lists of up to
// ES_MAX positions (longer ones take the sort form).  `lengths` (optional, with B): position p = t * B + b is padding
// when t >= lengths[b] -- its row is exactly zero (no gradient flows through padding) and it is skipped, as owner and as contributor:
// a ragged batch holds the pad id hundreds of times.
constexpr int ES_MAX = 4096;
// `fin(id, dim, d, sum)`: what the owner does with element d of the row's finished sum (common.h: RowAdd adds it into the dense gradient,
// RowSparseAdam updates the table and its moments in place -- embed_update = sparse); max_id: ids from there on are skipped.
template <class Fin>
__device__ __forceinline__ void embed_scatter_body(const Fin& fin, int64_t max_id, const int64_t* __restrict__ ids, int rows, int dim,
                                                   const float* __restrict__ dX, const int* __restrict__ lengths, int B) {
  __shared__ unsigned mask[ES_MAX / 32];
  __shared__ unsigned short list[ES_MAX];
  __shared__ int base[ES_MAX / 32 + 1];
  __shared__ int earlier;
  __shared__ float part[3][1024];
  const int p = blockIdx.x;
  const int64_t id = ids[p];
  auto padded = [&](int q) { return lengths != nullptr && (q / B) >= lengths[q % B]; };
  if (id < 0 || id >= max_id || padded(p)) return;       // block-uniform
  const int nwords = (rows + 31) / 32;
  if (threadIdx.x == 0) earlier = 0;
  for (int i = threadIdx.x; i < nwords; i += 256) mask[i] = 0u;
  __syncthreads();
  // one pass over the ids, eight loads in flight per thread
#pragma unroll 8
  for (int q = threadIdx.x; q < rows; q += 256)
    if (ids[q] == id && !padded(q)) atomicOr(&mask[q >> 5], 1u << (q & 31));
  __syncthreads();
  for (int i = threadIdx.x; i < (p + 31) / 32; i += 256) {      // an earlier position with this id owns it
    unsigned m = mask[i];
    if (32 * i + 32 > p) m &= (1u << (p - 32 * i)) - 1u;
    if (m) earlier = 1;                                  // benign race: every writer stores 1
  }
  __syncthreads();
  if (earlier) return;                                   // block-uniform
  // ordered list of the positions >= p that hold the id
  if (threadIdx.x == 0) {
    int c = 0;
    for (int i = p >> 5; i < nwords; ++i) {
      base[i] = c;
      unsigned m = mask[i];
      if (i == (p >> 5)) m &= ~((1u << (p & 31)) - 1u);
      c += __builtin_popcount(m);
    }
    base[nwords] = c;
  }
  __syncthreads();
  const int total = base[nwords];
  for (int i = (p >> 5) + threadIdx.x; i < nwords; i += 256) {
    unsigned m = mask[i];
    if (i == (p >> 5)) m &= ~((1u << (p & 31)) - 1u);
    int o = base[i];
    while (m) { list[o++] = (unsigned short)(32 * i + __builtin_ctz(m)); m &= m - 1; }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (total + 3) / 4;
  const int q0 = min(total, wave * per), q1 = min(total, q0 + per);
  for (int d0 = 0; d0 < dim; d0 += 256) {                // dimension groups of 256: lane handles d0 + lane + 64 j, j < 4
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = q0; q < q1; q += 8) {
      float v[8][4];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t r = list[min(q + u, q1 - 1)];      // (clamped: no load under a branch; the surplus is masked below)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int d = d0 + lane + 64 * j;
          v[u][j] = dX[r * dim + min(d, dim - 1)];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (q + u < q1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] += v[u][j];
        }
    }
    if (wave > 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) part[wave - 1][lane + 64 * j] = acc[j];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = d0 + lane + 64 * j;
        if (d < dim) fin(id, dim, d, ((acc[j] + part[0][lane + 64 * j]) + part[1][lane + 64 * j]) + part[2][lane + 64 * j]);
      }
    }
    __syncthreads();
  }
}
// fin.begin(): what a rule does once per launch (the dense rule records the step's scalars; the others nothing)
template <class Fin>
__global__ __launch_bounds__(256) void embed_short_kernel(Fin fin, int64_t max_id, const int64_t* __restrict__ ids, int n, int D,
                                                          const float* __restrict__ rows, const int* __restrict__ lengths, int B) {
  fin.begin();
  embed_scatter_body(fin, max_id, ids, n, D, rows, lengths, B);
}

// ---- the sort form
constexpr int CHUNK = 64;          // run boundaries = segment boundaries U multiples of CHUNK in the sorted list

__global__ void seg_keys_kernel(const int64_t* __restrict__ ids, int n, unsigned* keys, int* vals, const int* __restrict__ lengths, int B,
                                unsigned pad_key) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t id = ids[p];
  // negative ids (padding markers of the gathered lists) and, with `lengths`, the positions p = t * B + b past a sample's length
  // (their rows are exactly zero) sort to the end and are skipped
  const bool pad = id < 0 || (lengths != nullptr && (p / B) >= lengths[p % B]);
  keys[p] = (pad || (unsigned)id >= pad_key) ? pad_key : (unsigned)id;      // (pad_key: above every id; ids beyond it cannot be table rows)
  vals[p] = p;
}

__device__ __forceinline__ bool run_start(const unsigned* sid, int p) { return (p % CHUNK) == 0 || sid[p] != sid[p - 1]; }

// level 1: one wave per run start; part[p] = rows[pos[p]] + rows[pos[p+1]] + ... over the run, in list order.  A run that is its
// id's WHOLE segment (nearly all of them: a segment spans runs only across a chunk boundary) goes straight into the table row --
// the same bits level 2 would have produced from the one partial (0 + part, then the row's update) without the trip through `part`.
// `fin`: what a finished sum does (common.h: RowAdd -> the dense gradient row, RowSparseAdam -> the row's in-place update).
template <class Fin>
__device__ __forceinline__ void seg_level1_body(const Fin& fin, const unsigned* __restrict__ sid, const int* __restrict__ pos, int n, int D,
                                                const float* __restrict__ rows, float* part, unsigned pad_key) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= n) return;
  const unsigned id = sid[p];
  if (id == pad_key || !run_start(sid, p)) return;                 // wave-uniform
  int end = p + 1;
  const int lim = min(n, (p / CHUNK + 1) * CHUNK);
  while (end < lim && sid[end] == id) ++end;
  const bool whole = (p == 0 || sid[p - 1] != id) && (end == n || sid[end] != id);      // wave-uniform
  for (int c = lane; c < D; c += 64) {
    float acc = 0.f;
    int q = p;
    for (; q + 4 <= end; q += 4) {                                   // four independent loads in flight, added in list order
      const float a = rows[(int64_t)pos[q] * D + c], b = rows[(int64_t)pos[q + 1] * D + c];
      const float e = rows[(int64_t)pos[q + 2] * D + c], f = rows[(int64_t)pos[q + 3] * D + c];
      acc += a; acc += b; acc += e; acc += f;
    }
    for (; q < end; ++q) acc += rows[(int64_t)pos[q] * D + c];
    if (whole) fin((int64_t)id, D, c, acc);
    else part[(int64_t)p * D + c] = acc;
  }
}
template <class Fin>
__global__ __launch_bounds__(256) void seg_level1_kernel(Fin fin, const unsigned* __restrict__ sid, const int* __restrict__ pos, int n, int D,
                                                         const float* __restrict__ rows, float* part, unsigned pad_key) {
  fin.begin();
  seg_level1_body(fin, sid, pos, n, D, rows, part, pad_key);
}

// level 2: one wave per segment head; the sum of the segment's run partials, in list order, is the row's finished sum
template <class Fin>
__device__ __forceinline__ void seg_level2_body(const Fin& fin, const unsigned* __restrict__ sid, int n, int D, const float* __restrict__ part,
                                                unsigned pad_key) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= n) return;
  const unsigned id = sid[p];
  if (id == pad_key || (p > 0 && sid[p - 1] == id)) return;         // wave-uniform: not a segment head
  {
    const int q2 = (p / CHUNK + 1) * CHUNK;                          // a single run: level 1 finished the row itself
    if (q2 >= n || sid[q2] != id) return;
  }
  for (int c = lane; c < D; c += 64) {
    float acc = 0.f;
    for (int q = p; q < n && sid[q] == id; q = (q / CHUNK + 1) * CHUNK) acc += part[(int64_t)q * D + c];
    fin((int64_t)id, D, c, acc);
  }
}
// (no fin.begin(): level 1 of the same update has run it)
template <class Fin>
__global__ __launch_bounds__(256) void seg_level2_kernel(Fin fin, const unsigned* __restrict__ sid, int n, int D, const float* __restrict__ part,
                                                         unsigned pad_key) {
  seg_level2_body(fin, sid, n, D, part, pad_key);
}

// ---- embed_update = sparse under accumulation: a micro-batch's n = T B gradient rows (width D) and ids, appended at position `offset` of a
// list that outlives the workspace; the id of a padding position (t >= lengths[b], p = t B + b) becomes -1, which the rows update skips.
// vec: D % 4 == 0 and 16-byte aligned bases, so every row starts on a 16-byte boundary in both buffers (launch-uniform).
__global__ __launch_bounds__(256) void embed_rows_append_kernel(int64_t* ids_out, float* rows_out, int64_t offset,
                                                                const int64_t* __restrict__ ids, const float* __restrict__ rows, int n, int D,
                                                                const int* __restrict__ lengths, int B, int vec) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)n * D;
  float* dst = rows_out + offset * D;
  if (vec) {
    float4* d4 = reinterpret_cast<float4*>(dst);
    const float4* s4 = reinterpret_cast<const float4*>(rows);
    for (int64_t i = i0; i < (total >> 2); i += stride) d4[i] = s4[i];
  } else {
    for (int64_t i = i0; i < total; i += stride) dst[i] = rows[i];
  }
  for (int64_t p = i0; p < n; p += stride) {
    const bool pad = lengths != nullptr && (int)(p / B) >= lengths[p % B];
    ids_out[offset + p] = pad ? (int64_t)-1 : ids[p];
  }
}

// ---- embed_update = deferred (common.h: DenseRowArgs)
// updates a + 1 .. t of one row whose gradient was zero in all of them: adam1() with g = 0 and each update's own scalars, in order -- the
// calls the dense launches of those updates would have made.  One wave; a lane keeps up to RE elements of the row in registers, so the
// t - a dependent sqrt / div chains of a row run RE at a time.
constexpr int RE = 5;
__device__ __forceinline__ void replay_row(float* p, float* m, float* v, int D, int lane, int a, int t, const float* __restrict__ ring,
                                           int window, float b1, float b2, float eps) {
  a = max(a, max(t - window, 0));      // memory safety only: the hosts that count the updates (misa_step.hip, ops.py) flush before a row gets here
  for (int c0 = 0; c0 < D; c0 += 64 * RE) {
    float pe[RE], me[RE], ve[RE];
#pragma unroll
    for (int k = 0; k < RE; ++k) {
      const int c = c0 + 64 * k + lane;
      pe[k] = c < D ? p[c] : 0.f; me[k] = c < D ? m[c] : 0.f; ve[k] = c < D ? v[c] : 0.f;
    }
    for (int s = a + 1; s <= t; ++s) {
      const float step_size = ring[2 * (s % window)], inv_bc2_sqrt = ring[2 * (s % window) + 1];
#pragma unroll
      for (int k = 0; k < RE; ++k)
        if (c0 + 64 * k < D) adam1(pe[k], 0.f, me[k], ve[k], b1, b2, eps, INFINITY, 1.f, step_size, inv_bc2_sqrt);   // wave-uniform
    }
#pragma unroll
    for (int k = 0; k < RE; ++k) {
      const int c = c0 + 64 * k + lane;
      if (c < D) { p[c] = pe[k]; m[c] = me[k]; v[c] = ve[k]; }
    }
  }
}
// the rows of an id list, up to update `t`: one wave per position; the wave whose atomicMax raises row_step[id] owns the
// row for this launch (an integer claim: one writer per row, no float atomics), every other position of that id sees it current
__global__ __launch_bounds__(256) void embed_catch_up_kernel(float* P, float* M, float* V, int* row_step, const float* __restrict__ ring,
                                                             int window, const int64_t* __restrict__ ids, int n, int D,
                                                             const int* __restrict__ lengths, int B, int table_rows, float b1, float b2,
                                                             float eps, int t) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= n) return;
  const int64_t id = ids[p];
  if (id < 0 || id >= table_rows) return;                               // wave-uniform, as everything below
  if (lengths != nullptr && (p / B) >= lengths[p % B]) return;
  int a = 0;
  if (lane == 0) a = atomicMax(row_step + id, t);
  a = __shfl(a, 0);
  if (a >= t) return;
  const int64_t o = id * D;
  replay_row(P + o, M + o, V + o, D, lane, a, t, ring, window, b1, b2, eps);
}
// every stale row of the table, up to update `t`: one wave per row; a table with nothing stale is read (row_step) and not written
__global__ __launch_bounds__(256) void embed_flush_kernel(float* P, float* M, float* V, int* row_step, const float* __restrict__ ring,
                                                          int window, int D, int table_rows, float b1, float b2, float eps, int t) {
  const int lane = threadIdx.x & 63;
  for (int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6); row < table_rows; row += (int)gridDim.x * 4) {
    const int a = row_step[row];
    if (a >= t) continue;                                               // wave-uniform
    const int64_t o = (int64_t)row * D;
    replay_row(P + o, M + o, V + o, D, lane, a, t, ring, window, b1, b2, eps);
    if (lane == 0) row_step[row] = t;
  }
}
// a step that touches no row still leaves its scalars behind
__global__ void embed_step_record_kernel(DenseRowArgs ad) { dense_row_record(ad); }

// ---- host side: one list, one form decision, one launcher
// lists of this length take the sort form: the short form's scan costs n^2 / 256 id compares (B=256, T=50: 158 us against 9 us at B=32)
constexpr int ES_SORT_MIN = 3072;
static_assert(ES_SORT_MIN <= ES_MAX, "the scan form holds at most ES_MAX positions");

enum class ListForm { Short, Sort, Presorted };
// sort_always: the caller brought a work buffer sized for the sort form (mmda_embed_segment_sum), which its list takes however short
ListForm list_form(const unsigned* sorted, int n, bool sort_always) {
  if (sorted) return ListForm::Presorted;
  return sort_always || n >= ES_SORT_MIN ? ListForm::Sort : ListForm::Short;
}

// how ids become sort keys: pad_key, above every id that is updated (padding and ids from there on take it, sort to the end and are
// skipped), the key bits the sort walks, and the same bound for the short form
struct RowKeys { unsigned pad_key; int bits; int64_t max_id; };
constexpr RowKeys kAnyId{0xFFFFFFFFu, 32, INT64_MAX};
// ids lie in [0, table_rows): the sort walks the bits of table_rows only (two 8-bit passes at 20 000 rows instead of four)
RowKeys keys_of_table(int table_rows) {
  int bits = 1;
  while (bits < 32 && ((unsigned)table_rows >> bits) != 0u) ++bits;      // table_rows (the pad key) < 2^bits
  return {(unsigned)table_rows, bits, (int64_t)table_rows};
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct SegLayout { size_t keys_in, keys_out, vals_in, vals_out, part, cub, total, cub_bytes; };
SegLayout seg_layout(int n, int D) {
  SegLayout L{};
  size_t o = 0;
  L.keys_in = o; o += align256(sizeof(unsigned) * (size_t)n);
  L.keys_out = o; o += align256(sizeof(unsigned) * (size_t)n);
  L.vals_in = o; o += align256(sizeof(int) * (size_t)n);
  L.vals_out = o; o += align256(sizeof(int) * (size_t)n);
  L.part = o; o += align256(sizeof(float) * (size_t)n * D);
  size_t cb = 0;
  (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, cb, (const unsigned*)nullptr, (unsigned*)nullptr, (const int*)nullptr,
                                           (int*)nullptr, n, 0, 32, (hipStream_t)0);
  L.cub_bytes = cb;
  L.cub = o; o += align256(cb);
  L.total = o;
  return L;
}

// the sort form's buffers.  work.base: the caller's buffer (256-byte aligned, work.bytes of it); nullptr: the stream's scratch, ONE
// request (its result is only valid until the stream's next one), aligned here
struct RowWork { void* base; int64_t bytes; };
struct SegBuffers { unsigned* kin; unsigned* kout; int* vin; int* vout; float* part; void* cub; size_t cub_bytes; };
int seg_carve(SegBuffers* b, int n, int D, const RowWork& work, hipStream_t s) {
  const SegLayout L = seg_layout(n, D);
  unsigned char* w = (unsigned char*)work.base;
  if (w) {
    if (work.bytes < (int64_t)L.total || ((uintptr_t)w & 255)) return MMDA_EINVAL;
  } else {
    float* scratch = mmda_scratch_get(s, L.total + 256);
    if (!scratch) return MMDA_ELAUNCH;
    w = (unsigned char*)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
  }
  *b = SegBuffers{(unsigned*)(w + L.keys_in), (unsigned*)(w + L.keys_out), (int*)(w + L.vals_in), (int*)(w + L.vals_out),
                  (float*)(w + L.part), (void*)(w + L.cub), L.cub_bytes};
  return MMDA_OK;
}

// the sorted (key, position) list of an id list: kout / vout (n words each); kin / vin / cub: temporaries
int seg_sort(const int64_t* ids, int n, const int* lengths, int B, const RowKeys& keys, unsigned* kin, int* vin, unsigned* kout, int* vout,
             void* cub, size_t cub_bytes, hipStream_t s) {
  hipLaunchKernelGGL(seg_keys_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, ids, n, kin, vin, lengths, B, keys.pad_key);
  MMDA_CHECK_LAUNCH("mmda_embed_segment_sum/keys");
  size_t cb = cub_bytes;
  // LSD radix sort: stable, so equal ids keep their list order (the order every rank sums them in)
  if (hipcub::DeviceRadixSort::SortPairs(cub, cb, kin, kout, vin, vout, n, 0, keys.bits, s) != hipSuccess) {
    mmda_set_error("mmda_embed_segment_sum/sort", hipGetLastError());
    return MMDA_ELAUNCH;
  }
  return MMDA_OK;
}

// Rule `fin` over list `l` in the form the list takes, on stream s.  The rule's own pointers are the caller's to check.  `what` names
// the entry in a launch error.
template <class Fin>
int embed_rows_apply(const Fin& fin, const RowKeys& keys, const EmbedList& l, const RowWork& work, hipStream_t s, const char* what) {
  const bool own_work = work.base != nullptr;
  const ListForm form = list_form(l.sorted, l.n, own_work);
  if (!l.rows || l.n < 0 || l.D <= 0 || (l.lengths && l.B <= 0) || (form != ListForm::Presorted && !l.ids)) return MMDA_EINVAL;
  // the short form keeps a row of at most 1024 floats in LDS: refused for every list that could have taken it, whatever its length
  if (!own_work && l.D > 1024) return MMDA_EINVAL;
  if (l.n == 0) return MMDA_OK;
  auto launched = [&](const char* stage) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return true;
    char name[96];
    snprintf(name, sizeof(name), "%s%s", what, stage);
    mmda_set_error(name, e);
    return false;
  };
  if (form == ListForm::Short) {
    hipLaunchKernelGGL(embed_short_kernel<Fin>, dim3(l.n), dim3(256), 0, s, fin, keys.max_id, l.ids, l.n, l.D, l.rows, l.lengths, l.B);
    return launched("") ? MMDA_OK : MMDA_ELAUNCH;
  }
  const unsigned* sid;
  const int* pos;
  float* part;
  if (form == ListForm::Presorted) {
    sid = l.sorted; pos = reinterpret_cast<const int*>(l.sorted + l.n);
    part = mmda_scratch_get(s, sizeof(float) * (size_t)l.n * l.D);
    if (!part) return MMDA_ELAUNCH;
  } else {
    // sort, then the sums: one piece of memory holds the sort's buffers and the run partials
    SegBuffers b;
    int rc = seg_carve(&b, l.n, l.D, work, s);
    if (!rc) rc = seg_sort(l.ids, l.n, l.lengths, l.B, keys, b.kin, b.vin, b.kout, b.vout, b.cub, b.cub_bytes, s);
    if (rc) return rc;
    sid = b.kout; pos = b.vout; part = b.part;
  }
  hipLaunchKernelGGL(seg_level1_kernel<Fin>, dim3(ceil_div(l.n, 4)), dim3(256), 0, s, fin, sid, pos, l.n, l.D, l.rows, part, keys.pad_key);
  if (!launched("/level1")) return MMDA_ELAUNCH;
  hipLaunchKernelGGL(seg_level2_kernel<Fin>, dim3(ceil_div(l.n, 4)), dim3(256), 0, s, fin, sid, l.n, l.D, part, keys.pad_key);
  return launched("/level2") ? MMDA_OK : MMDA_ELAUNCH;
}

}  // namespace

int mmda_embed_gather_stamped(const float* W, const int64_t* ids, int rows, int dim, float* out, const RowStamp* st, void* stream) {
  if (!W || !ids || !out || rows < 0 || dim <= 0) return MMDA_EINVAL;
  if (st && (!st->stamp || st->ids != ids || st->n != rows || st->table_rows <= 0 || rows == 0)) return MMDA_EINVAL;
  if (rows == 0) return MMDA_OK;
  hipLaunchKernelGGL(embed_gather_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, W, ids, rows, dim, out,
                     st ? st->stamp : nullptr, st ? st->epoch : 0u, st ? st->table_rows : 0);
  MMDA_CHECK_LAUNCH("mmda_embed_gather");
  return MMDA_OK;
}
extern "C" int mmda_embed_gather(const float* W, const int64_t* ids, int rows, int dim, float* out, void* stream) {
  return mmda_embed_gather_stamped(W, ids, rows, dim, out, nullptr, stream);
}

// ---- RowAdd: the dense gradient
bool mmda_embed_scatter_sorts(int rows) { return list_form(nullptr, rows, false) == ListForm::Sort; }

// (internal, misa_backward.hip) dW[id] += the list-order sum of the id's rows.  A sorted list has table_rows as its pad key
// (mmda_embed_sort_ids); an unsorted one is keyed here with no bound on its ids, all 32 key bits
int mmda_embed_list_add(float* dW, const EmbedList& l, int table_rows, void* stream) {
  const bool presorted = list_form(l.sorted, l.n, false) == ListForm::Presorted;
  if (!dW || (presorted && table_rows <= 0)) return MMDA_EINVAL;
  return embed_rows_apply(RowAdd{dW, 1}, presorted ? keys_of_table(table_rows) : kAnyId, l, RowWork{}, (hipStream_t)stream,
                          "mmda_embed_scatter_add");
}

extern "C" int mmda_embed_scatter_add(float* dW, const int64_t* ids, int rows, int dim, const float* dX, void* stream) {
  if (!dW || !ids || !dX || rows < 0 || dim <= 0 || dim > 1024) return MMDA_EINVAL;
  if (rows == 0) return MMDA_OK;
  return mmda_embed_list_add(dW, EmbedList{ids, nullptr, rows, dim, dX, nullptr, 0}, 0, stream);
}

extern "C" int64_t mmda_embed_segment_sum_work_bytes(int n, int D) {
  if (n < 0 || D <= 0) return MMDA_EINVAL;
  if (n == 0) return 256;
  return (int64_t)seg_layout(n, D).total;
}

// dW[id] = the list-order sum (accumulate = 0): the sort form whatever the length, in the caller's work buffer, rows of any width
extern "C" int mmda_embed_segment_sum(float* dW, const int64_t* ids, int n, int D, const float* rows, void* work, int64_t work_bytes,
                                      void* stream) {
  if (!dW || !work) return MMDA_EINVAL;
  return embed_rows_apply(RowAdd{dW, 0}, kAnyId, EmbedList{ids, nullptr, n, D, rows, nullptr, 0}, RowWork{work, work_bytes},
                          (hipStream_t)stream, "mmda_embed_segment_sum");
}

// ---- the sorted list on its own (internal, misa_backward.hip): it depends on the ids only, so a training step makes it early, beside a
// recurrence, and only the sums wait for the gradient rows.  `sorted`: 2 n words the caller keeps (keys, then positions);
// table_rows: ids lie in [0, table_rows).
int mmda_embed_sort_ids(const int64_t* ids, int n, const int* lengths, int B, int table_rows, unsigned* sorted, void* stream) {
  if (!ids || !sorted || n < 0 || table_rows <= 0 || (lengths && B <= 0)) return MMDA_EINVAL;
  if (n == 0) return MMDA_OK;
  SegBuffers b;
  const int rc = seg_carve(&b, n, 1, RowWork{}, (hipStream_t)stream);
  if (rc) return rc;
  return seg_sort(ids, n, lengths, B, keys_of_table(table_rows), b.kin, b.vin, sorted, reinterpret_cast<int*>(sorted + n), b.cub,
                  b.cub_bytes, (hipStream_t)stream);
}

// ---- RowSparseAdam (embed_update = sparse): the row update where a row's sum becomes final.  The pad key is the table's row count:
// ids from there on are never updated.
// the scalars of one SparseAdam step.  torch.optim.SparseAdam: step_size = lr sqrt(1 - b2^t) / (1 - b1^t), in double here,
// once per step (the dense launch keeps its two scalars lr / bc1 and 1 / sqrt(bc2): its eps sits elsewhere)
int mmda_sparse_adam_args(SparseAdamArgs* out, float* P, float* M, float* V, int table_rows, float lr, float beta1, float beta2, float eps,
                          float clip, float grad_scale, int step) {
  if (!out || !P || !M || !V || table_rows <= 0 || step < 1) return MMDA_EINVAL;
  const BiasCorrections c = bias_corrections(beta1, beta2, step);
  *out = SparseAdamArgs{P, M, V, table_rows, beta1, beta2, eps, clip, grad_scale, (float)((double)lr * sqrt(c.bc2) / c.bc1)};
  return MMDA_OK;
}

int mmda_embed_list_sparse_adam(const SparseAdamArgs& ad, const EmbedList& l, void* stream) {
  if (ad.table_rows <= 0) return MMDA_EINVAL;
  return embed_rows_apply(RowSparseAdam{ad}, keys_of_table(ad.table_rows), l, RowWork{}, (hipStream_t)stream, "mmda_embed_rows_sparse_adam");
}

extern "C" int mmda_embed_rows_sparse_adam(float* P, float* M, float* V, const int64_t* ids, int n, int D, const float* rows,
                                           const int32_t* lengths, int B, int table_rows, float lr, float beta1, float beta2, float eps,
                                           float clip, float grad_scale, int step, void* stream) {
  if (!ids || !rows || n < 0 || D <= 0 || D > 1024 || (lengths && B <= 0)) return MMDA_EINVAL;
  SparseAdamArgs ad;
  const int rc = mmda_sparse_adam_args(&ad, P, M, V, table_rows, lr, beta1, beta2, eps, clip, grad_scale, step);
  if (rc) return rc;
  return mmda_embed_list_sparse_adam(ad, EmbedList{ids, nullptr, n, D, rows, lengths, B}, stream);
}

extern "C" int mmda_embed_rows_append(int64_t* ids_out, float* rows_out, int64_t offset, int64_t capacity, const int64_t* ids,
                                      const float* rows, int n, int D, const int32_t* lengths, int B, void* stream) {
  if (!ids_out || !rows_out || !ids || !rows || n < 0 || D <= 0 || offset < 0 || capacity < 0 || (lengths && B <= 0)) return MMDA_EINVAL;
  if (offset > capacity || (int64_t)n > capacity - offset) return MMDA_EINVAL;                 // the list must hold the rows
  if (((uintptr_t)ids_out | (uintptr_t)ids) & 7 || ((uintptr_t)rows_out | (uintptr_t)rows) & 3) return MMDA_EINVAL;
  if (n == 0) return MMDA_OK;
  const int vec = (D & 3) == 0 && (((uintptr_t)rows_out | (uintptr_t)rows) & 15) == 0;
  const int64_t work = vec ? ((int64_t)n * D) >> 2 : (int64_t)n * D;
  hipLaunchKernelGGL(embed_rows_append_kernel, dim3(stream_blocks(work)), dim3(256), 0, (hipStream_t)stream, ids_out, rows_out, offset, ids, rows, n,
                     D, lengths, B, vec);
  MMDA_CHECK_LAUNCH("mmda_embed_rows_append");
  return MMDA_OK;
}

// ---- RowDenseAdam (embed_update = deferred): host side
extern "C" int64_t mmda_embed_deferred_scalar_floats(int window) { return window < 1 ? MMDA_EINVAL : 2 * (int64_t)window; }

extern "C" int mmda_embed_deferred_reset(int32_t* row_step, int table_rows, void* stream) {
  if (!row_step || table_rows <= 0) return MMDA_EINVAL;
  if (hipMemsetAsync(row_step, 0, sizeof(int32_t) * (size_t)table_rows, (hipStream_t)stream) != hipSuccess) return MMDA_ELAUNCH;
  return MMDA_OK;
}

static bool deferred_state_ok(const float* P, const float* M, const float* V, const int32_t* row_step, const float* step_scalars, int window,
                              int D, int table_rows) {
  return P && M && V && row_step && step_scalars && window >= 1 && D > 0 && D <= 1024 && table_rows > 0;
}

extern "C" int mmda_embed_rows_catch_up(float* P, float* M, float* V, int32_t* row_step, const float* step_scalars, int window,
                                        const int64_t* ids, int n, int D, const int32_t* lengths, int B, int table_rows, float beta1,
                                        float beta2, float eps, int upto, void* stream) {
  if (!deferred_state_ok(P, M, V, row_step, step_scalars, window, D, table_rows) || !ids || n < 0 || (lengths && B <= 0) || upto < 0)
    return MMDA_EINVAL;
  if (n == 0 || upto == 0) return MMDA_OK;
  hipLaunchKernelGGL(embed_catch_up_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, (hipStream_t)stream, P, M, V, row_step, step_scalars, window,
                     ids, n, D, lengths, B, table_rows, beta1, beta2, eps, upto);
  MMDA_CHECK_LAUNCH("mmda_embed_rows_catch_up");
  return MMDA_OK;
}

extern "C" int mmda_embed_rows_flush(float* P, float* M, float* V, int32_t* row_step, const float* step_scalars, int window, int D,
                                     int table_rows, float beta1, float beta2, float eps, int upto, void* stream) {
  if (!deferred_state_ok(P, M, V, row_step, step_scalars, window, D, table_rows) || upto < 0) return MMDA_EINVAL;
  if (upto == 0) return MMDA_OK;
  int blocks = ceil_div(table_rows, 4);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(embed_flush_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, M, V, row_step, step_scalars, window, D,
                     table_rows, beta1, beta2, eps, upto);
  MMDA_CHECK_LAUNCH("mmda_embed_rows_flush");
  return MMDA_OK;
}

// internal (misa_step.hip): update number `seq` (the count of updates since the reset, last + 1), made with Adam step number `step`, for
// the rows of an id list.  Counts that are multiples of the window flush the table first: the slot this update's scalars take is then
// needed by no row.  catch_up: bring the list's rows to seq - 1 first (a forward of the same
// batch has done so already inside a training step).  sorted != nullptr: the list as mmda_embed_sort_ids left it.
int mmda_embed_dense_adam_apply(float* P, float* M, float* V, int32_t* row_step, float* step_scalars, int window, const int64_t* ids,
                                const unsigned* sorted, int n, int D, const float* rows, const int32_t* lengths, int B, int table_rows,
                                float lr, float beta1, float beta2, float eps, float clip, float grad_scale, int seq, int step,
                                bool catch_up, void* stream) {
  if (!deferred_state_ok(P, M, V, row_step, step_scalars, window, D, table_rows) || !ids || !rows || n < 0 || (lengths && B <= 0) ||
      step < 1 || seq < 1)
    return MMDA_EINVAL;
  const AdamStepScalars sc = adam_step_scalars(lr, beta1, beta2, step);                      // the dense launch's two scalars
  const DenseRowArgs ad{P, M, V, row_step, step_scalars, window, table_rows, beta1, beta2, eps, clip, grad_scale, sc.step_size,
                        sc.inv_bc2_sqrt, seq};
  int rc = MMDA_OK;
  if (seq % window == 0)
    rc = mmda_embed_rows_flush(P, M, V, row_step, step_scalars, window, D, table_rows, beta1, beta2, eps, seq - 1, stream);
  else if (catch_up)
    rc = mmda_embed_rows_catch_up(P, M, V, row_step, step_scalars, window, ids, n, D, lengths, B, table_rows, beta1, beta2, eps, seq - 1,
                                  stream);
  if (rc) return rc;
  if (n == 0) {
    hipLaunchKernelGGL(embed_step_record_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ad);
    MMDA_CHECK_LAUNCH("mmda_embed_rows_dense_adam/record");
    return MMDA_OK;
  }
  return embed_rows_apply(RowDenseAdam{ad}, keys_of_table(table_rows), EmbedList{ids, sorted, n, D, rows, lengths, B}, RowWork{},
                          (hipStream_t)stream, "mmda_embed_rows_dense_adam");
}

extern "C" int mmda_embed_rows_dense_adam(float* P, float* M, float* V, int32_t* row_step, float* step_scalars, int window,
                                          const int64_t* ids, int n, int D, const float* rows, const int32_t* lengths, int B,
                                          int table_rows, float lr, float beta1, float beta2, float eps, float clip, float grad_scale,
                                          int seq, int step, void* stream) {
  return mmda_embed_dense_adam_apply(P, M, V, row_step, step_scalars, window, ids, nullptr, n, D, rows, lengths, B, table_rows, lr, beta1,
                                     beta2, eps, clip, grad_scale, seq, step, true, stream);
}
