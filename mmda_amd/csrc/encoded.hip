// Encoder cache (mmda_amd/encoded.py: EncoderCache, EncodedLoader): with the encoders frozen a sample's three utterance vectors
// utt_t (4 H_t), utt_v (4 H_v), utt_a (4 H_a) -- all the fusion block reads of the encoders -- are constants.  They are computed once,
// kept in tables of one row per SAMPLE, and every later step starts at the projections: collect copies what an evaluation forward left
// in the workspace into the tables (one launch per batch of the build), gather copies B table rows into the workspace (one launch per
// step).  Row movers in the style of infer.hip and collate.hip.  DESIGN.md 4g.
#include "internal.h"

namespace {

// blockIdx.y: 0, 1, 2 = the utterance rows of t, v, a; 3 = the label row (gather only)
constexpr int ENC_SEGS = 4;

struct EncodedArgs {
  const float* src[ENC_SEGS]; float* dst[ENC_SEGS];
  int w[ENC_SEGS], vec[ENC_SEGS];          // row width in floats; the 16-byte form (host: w % 4 == 0, both bases 16-byte aligned)
  const int32_t* idx; int64_t base; int B;
};

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

// One wave per (batch column b, segment), lanes along the row; the four waves of a workgroup take four adjacent columns.  A wave reads
// its table row index once, so both addresses of its row are known up front; offsets are 64-bit (a table of 2^20 samples x 1200 floats
// is past 2^31 bytes).  GATHER: table row idx[b] -> batch row b (repeats allowed: the tables are only read).  Otherwise batch row b ->
// table row idx[b], or base + b without an index list (the host guarantees rows in range and distinct, as for infer_collect_kernel).
// Copies only: no atomics, no LDS, no scratch.
template <bool GATHER>
__global__ __launch_bounds__(256) void encoded_rows_kernel(const EncodedArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;                                      // wave-uniform
  const int seg = (int)blockIdx.y;
  if (!a.dst[seg]) return;                                   // segment not requested
  const int64_t r = a.idx ? (int64_t)a.idx[b] : a.base + b;
  const int64_t w = a.w[seg];
  const float* src = a.src[seg] + (GATHER ? r : (int64_t)b) * w;
  float* dst = a.dst[seg] + (GATHER ? (int64_t)b : r) * w;
  if (a.vec[seg]) copy_row<true>(src, dst, (int)w, lane); else copy_row<false>(src, dst, (int)w, lane);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// segment k of a launch: both pointers (requested, with a positive width) or neither (skipped); false for anything else
bool set_segment(EncodedArgs& a, int k, const float* src, float* dst, int w) {
  a.src[k] = nullptr; a.dst[k] = nullptr; a.w[k] = 0; a.vec[k] = 0;
  if (!src && !dst) return true;
  if (!src || !dst || w <= 0) return false;
  a.src[k] = src; a.dst[k] = dst; a.w[k] = w;
  // a row's offset is a multiple of its width, so a width of whole float4s and two aligned bases make every row 16-byte aligned
  a.vec[k] = (w % 4) == 0 && aligned16(src) && aligned16(dst);
  return true;
}

}  // namespace

extern "C" int mmda_encoded_collect(const float* utt_t, const float* utt_v, const float* utt_a, int wt, int wv, int wa, float* tab_t,
                                    float* tab_v, float* tab_a, const int32_t* dst, int64_t base, int B, void* stream) {
  if (B <= 0) return MMDA_EINVAL;
  if (!tab_t && !tab_v && !tab_a) return MMDA_EINVAL;
  EncodedArgs a;
  if (!set_segment(a, 0, utt_t, tab_t, wt) || !set_segment(a, 1, utt_v, tab_v, wv) || !set_segment(a, 2, utt_a, tab_a, wa)) return MMDA_EINVAL;
  set_segment(a, 3, nullptr, nullptr, 0);
  a.idx = dst; a.base = base; a.B = B;
  hipLaunchKernelGGL(encoded_rows_kernel<false>, dim3(ceil_div(B, 4), 3), dim3(256), 0, (hipStream_t)stream, a);
  MMDA_CHECK_LAUNCH("mmda_encoded_collect");
  return MMDA_OK;
}

extern "C" int mmda_encoded_gather(const float* tab_t, const float* tab_v, const float* tab_a, int wt, int wv, int wa,
                                   const float* tab_emo, int ncls, const int32_t* rows, int B, float* utt_t, float* utt_v, float* utt_a,
                                   float* emo, void* stream) {
  if (B <= 0 || !rows) return MMDA_EINVAL;
  if (!utt_t && !utt_v && !utt_a && !emo) return MMDA_EINVAL;
  EncodedArgs a;
  if (!set_segment(a, 0, tab_t, utt_t, wt) || !set_segment(a, 1, tab_v, utt_v, wv) || !set_segment(a, 2, tab_a, utt_a, wa) ||
      !set_segment(a, 3, tab_emo, emo, ncls))
    return MMDA_EINVAL;
  a.idx = rows; a.base = 0; a.B = B;
  hipLaunchKernelGGL(encoded_rows_kernel<true>, dim3(ceil_div(B, 4), emo ? 4 : 3), dim3(256), 0, (hipStream_t)stream, a);
  MMDA_CHECK_LAUNCH("mmda_encoded_gather");
  return MMDA_OK;
}
