// Inference pass on the device (mmda_amd/inference.py: InferencePass): what one evaluation forward left in the workspace -- one batch,
// columns in the loader's length-sorted order -- copied into result tables that hold one row per SAMPLE, in one launch per batch.
// The reference names the pass three times and builds none of it (src/inference.py is a TODO, utils/tools.py:save_hidden wants the
// per-sample h, models.py:159 asks how to get at the attention scores).
#include "internal.h"

namespace {

struct InferArgs {
  mmda_infer_src s; mmda_infer_out o;
  const int32_t* dst; int64_t base; int B;
  int vec_hidden, vec_utt;                 // the 16-byte form of the two wide rows (host: width % 4 == 0, both bases 16-byte aligned)
};

// blockIdx.y: 0 = the narrow rows (scores, labels, tcp, attention), 1 = hidden, 2 .. 7 = token k = y - 2 of utterance
constexpr int INFER_SEGS = 8;

template <bool VEC>
__device__ __forceinline__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, int n, int lane) {
  if (VEC) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int c = lane; c < (n >> 2); c += 64) d4[c] = s4[c];
  } else {
    for (int c = lane; c < n; c += 64) dst[c] = src[c];
  }
}

// One wave per batch column b, lanes along a row; the four waves of a workgroup take four adjacent columns; blockIdx.y picks the field.
// A wave reads its row index once (dst[b], or base + b), so every address of its segment is known up front.  Source layouts, as the
// forward leaves them (misa_forward.hip):
//   scores / labels (B, C), tcp (B, 6): row b.
//   hfused: LayerNorm 2 runs over rows (s, b) of the (6, B, hs) token block and writes them PERMUTED -- norm2_fwd sets permute_S = 6,
//     permute_B = B, so row (s * B + b) lands at b * 6 hs + s * hs -- and the head GEMM reads the result as (B, 6 hs) with lda = 6 hs.
//     Row b of hfused therefore already is the reference's h = cat(h[0..5], dim=1) of sample b: `hidden` is a plain row copy.
//   x6 (6, B, hs): token-major, [private t, v, a, shared t, v, a]; utterance[r][k] = x6[k][b], a transposing gather of six rows.
//   probs (B, nhead, 6, 6): the softmax rows before attention dropout, written in every mode; attention[r] is their head average,
//     summed in head order in fp32 and divided by nhead (what nn.MultiheadAttention(need_weights=True) returns).
// hs = 128 rows and the 6 hs hidden row move as 16-byte lanes; C = 6, the 36 attention floats and odd hs as 4-byte lanes (consecutive
// lanes on consecutive floats either way).  Copies and one add per head: no atomics, no LDS, no scratch.  Nothing checks r.
__global__ __launch_bounds__(256) void infer_collect_kernel(const InferArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;                                      // wave-uniform
  const int seg = (int)blockIdx.y;
  const int64_t r = a.dst ? (int64_t)a.dst[b] : a.base + b;
  const int C = a.s.ncls, hs = a.s.hs;
  if (seg == 0) {
    if (a.o.scores) copy_row<false>(a.s.scores + (int64_t)b * C, a.o.scores + r * C, C, lane);
    if (a.o.labels) copy_row<false>(a.s.labels + (int64_t)b * C, a.o.labels + r * C, C, lane);
    if (a.o.tcp) copy_row<false>(a.s.tcp + (int64_t)b * 6, a.o.tcp + r * 6, 6, lane);
    if (a.o.attention) {
      const int nhead = a.s.nhead;
      const float* p = a.s.probs + (int64_t)b * nhead * 36;
      float* out = a.o.attention + r * 36;
      for (int e = lane; e < 36; e += 64) {
        float acc = p[e];
        for (int h = 1; h < nhead; ++h) acc += p[(int64_t)h * 36 + e];
        out[e] = acc / (float)nhead;
      }
    }
  } else if (seg == 1) {
    if (!a.o.hidden) return;
    const float* src = a.s.hfused + (int64_t)b * 6 * hs;
    float* out = a.o.hidden + r * 6 * hs;
    if (a.vec_hidden) copy_row<true>(src, out, 6 * hs, lane); else copy_row<false>(src, out, 6 * hs, lane);
  } else {
    if (!a.o.utterance) return;
    const int k = seg - 2;
    const float* src = a.s.x6 + ((int64_t)k * a.B + b) * hs;
    float* out = a.o.utterance + (r * 6 + k) * hs;
    if (a.vec_utt) copy_row<true>(src, out, hs, lane); else copy_row<false>(src, out, hs, lane);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int mmda_infer_collect(const mmda_infer_src* src, const mmda_infer_out* out, const int32_t* dst, int64_t base, int B,
                                  void* stream) {
  if (!src || !out || B <= 0) return MMDA_EINVAL;
  if (src->ncls <= 0 || src->hs <= 0 || src->nhead <= 0) return MMDA_EINVAL;
  if (!out->scores && !out->labels && !out->tcp && !out->hidden && !out->utterance && !out->attention) return MMDA_EINVAL;
  if ((out->scores && !src->scores) || (out->labels && !src->labels) || (out->tcp && !src->tcp) || (out->hidden && !src->hfused) ||
      (out->utterance && !src->x6) || (out->attention && !src->probs))
    return MMDA_EINVAL;
  InferArgs a;
  a.s = *src; a.o = *out; a.dst = dst; a.base = base; a.B = B;
  // a row's offset is a multiple of its width, so a width of whole float4s and two aligned bases make every row 16-byte aligned
  a.vec_hidden = out->hidden && (6 * src->hs) % 4 == 0 && aligned16(src->hfused) && aligned16(out->hidden);
  a.vec_utt = out->utterance && src->hs % 4 == 0 && aligned16(src->x6) && aligned16(out->utterance);
  hipLaunchKernelGGL(infer_collect_kernel, dim3(ceil_div(B, 4), INFER_SEGS), dim3(256), 0, (hipStream_t)stream, a);
  MMDA_CHECK_LAUNCH("mmda_infer_collect");
  return MMDA_OK;
}
