// Batch collation on the device (mmda_amd/data.py: DeviceLoader): the dataset lives in HBM as three flat position-major arrays, and a
// batch -- the reference's time-major pad_sequence tensors (data_loader.py:59-122) -- is one gather by B sample indices.
#include "internal.h"

// One wave per batch column b, lanes along the feature dimension; blockIdx.y strides over the time positions.  A wave reads its sample's
// index and extent once, so inside the t loop every address is known up front and the loads of consecutive positions are independent.
// Rows are dv / da floats wide (35 and 74 on MOSEI: no 16-byte multiples), so every access is 4 bytes per lane, consecutive lanes on
// consecutive floats: a row is one contiguous segment on both sides, and the four waves of a block write four adjacent output rows.
// Positions past a sample's length get pad_id / zeros from the same launch (t < len is wave-uniform): the outputs need no memset.
__global__ __launch_bounds__(256) void collate_gather_kernel(const int32_t* __restrict__ words, const float* __restrict__ visual,
                                                             const float* __restrict__ acoustic, const int64_t* __restrict__ offsets,
                                                             const float* __restrict__ emo, const float* __restrict__ sentiment,
                                                             const int32_t* __restrict__ order, int B, int T, int dv, int da, int pad_id,
                                                             int64_t* __restrict__ out_ids, float* __restrict__ out_v,
                                                             float* __restrict__ out_a, float* __restrict__ out_emo,
                                                             float* __restrict__ out_y) {
  const int lane = threadIdx.x & 63;
  const int b = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;                                        // wave-uniform
  const int64_t s = order[b];
  const int64_t o0 = offsets[s];
  const int64_t len = offsets[s + 1] - o0;
  if (blockIdx.y == 0) {                                     // the labels of the column, once
    if (out_emo && lane < 6) out_emo[(int64_t)b * 6 + lane] = emo[s * 6 + lane];
    if (lane == 6) out_y[b] = sentiment[s];
  }
  for (int t = (int)blockIdx.y; t < T; t += (int)gridDim.y) {
    const int64_t dst = (int64_t)t * B + b;
    if (t < len) {
      const int64_t src = o0 + t;
      for (int c = lane; c < dv; c += 64) out_v[dst * dv + c] = visual[src * dv + c];
      for (int c = lane; c < da; c += 64) out_a[dst * da + c] = acoustic[src * da + c];
      if (lane == 0) out_ids[dst] = (int64_t)words[src];
    } else {
      for (int c = lane; c < dv; c += 64) out_v[dst * dv + c] = 0.f;
      for (int c = lane; c < da; c += 64) out_a[dst * da + c] = 0.f;
      if (lane == 0) out_ids[dst] = (int64_t)pad_id;
    }
  }
}

extern "C" int mmda_collate_gather(const int32_t* words, const float* visual, const float* acoustic, const int64_t* offsets,
                                   const float* emo, const float* sentiment, const int32_t* order, int B, int T, int dv, int da,
                                   int pad_id, int64_t* out_ids, float* out_v, float* out_a, float* out_emo, float* out_y, void* stream) {
  if (!words || !visual || !acoustic || !offsets || !sentiment || !order || !out_ids || !out_v || !out_a || !out_y) return MMDA_EINVAL;
  if (B <= 0 || T <= 0 || dv <= 0 || da <= 0) return MMDA_EINVAL;
  if (!emo && out_emo) return MMDA_EINVAL;
  const int bx = ceil_div(B, 4);
  int by = 2048 / bx;                                        // about 2048 workgroups (8 per CU) at the most; the t loop takes the rest
  if (by < 1) by = 1;
  if (by > T) by = T;
  hipLaunchKernelGGL(collate_gather_kernel, dim3(bx, by), dim3(256), 0, (hipStream_t)stream, words, visual, acoustic, offsets, emo,
                     sentiment, order, B, T, dv, da, pad_id, out_ids, out_v, out_a, out_emo, out_y);
  MMDA_CHECK_LAUNCH("mmda_collate_gather");
  return MMDA_OK;
}
