// Squared-norm head objective of the MAS importance pass: J = mean_b( sum_t |z[b,t]|^2 / max(count_b, 1e-13) ) over
// the rows whose shifted label is a token -- the rows and the normaliser of the cross-entropy (ce.hip); the label values are never used.
// HBM-bound: one 256-thread block per (b,t) row, 4-element vector loads, fp32 accumulation; no atomics, the same bits on every call.
#include "common.h"

namespace mafed {

// row (b,t) is labelled when its shifted label labels[b,t+1] is not the ignore index; the last position predicts nothing
__device__ __forceinline__ bool sqnorm_labelled(const int64_t* __restrict__ labels, int b, int t, int Tn) {
  return t < Tn - 1 && labels[(int64_t)b * Tn + t + 1] != -100;
}

template <typename T>
__global__ __launch_bounds__(256) void sqnorm_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels, int B, int Tn,
                                                         int64_t V, float* __restrict__ rowsq) {
  __shared__ float sm[4];
  const int64_t r = blockIdx.x;
  const int b = (int)(r / Tn), t = (int)(r - (int64_t)b * Tn);
  if (!sqnorm_labelled(labels, b, t, Tn)) {   // (block-uniform)
    if (threadIdx.x == 0) rowsq[r] = 0.f;
    return;
  }
  const T* x = logits + r * V;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll 4   // four loads in flight per thread: the sparse head's 256 rows are one block per CU
  for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) {
    const float4 v = load4(x + c);
    s0 += v.x * v.x + v.y * v.y;
    s1 += v.z * v.z + v.w * v.w;
  }
  const float s = block_sum<256>(s0 + s1, sm);
  if (threadIdx.x == 0) rowsq[r] = s;
}

// out = mean_b( sum_t rowsq[b,t] / max(count_b, 1e-13) ) as in ce_finalize_kernel: one wave per sample, fixed-order sums.
// `poison` (may be null): a non-zero device flag turns the result into NaN (mafed_ce_fwd_guarded).
__global__ __launch_bounds__(256) void sqnorm_finalize_kernel(const float* __restrict__ rowsq, const int64_t* __restrict__ labels, int B, int Tn,
                                                              float* __restrict__ out, const int* __restrict__ poison) {
  __shared__ float sm[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc = 0.f;
  for (int b = wave; b < B; b += 4) {
    float s = 0.f, c = 0.f;
    for (int t = lane; t < Tn - 1; t += 64) {
      if (sqnorm_labelled(labels, b, t, Tn)) { c += 1.f; s += rowsq[(int64_t)b * Tn + t]; }
    }
    s = wave_sum(s);
    c = wave_sum(c);
    acc += s / fmaxf(c, 1e-13f);
  }
  if (lane == 0) sm[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float j = ((sm[0] + sm[1]) + (sm[2] + sm[3])) / (float)B;
    out[0] = (poison && poison[0] != 0) ? __int_as_float(0x7fc00000) : j;
  }
}

// dJ/dz = 2 z dloss / (B max(count_b, 1e-13)) on labelled rows, zeros elsewhere; dlogits is a buffer of its own
template <typename T>
__global__ __launch_bounds__(256) void sqnorm_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels, int B, int Tn, int64_t V,
                                                         const float* __restrict__ dloss, T* __restrict__ dlogits) {
  const int64_t r = blockIdx.x;
  const int b = (int)(r / Tn), t = (int)(r - (int64_t)b * Tn);
  const T* x = logits + r * V;
  T* dx = dlogits + r * V;
  if (!sqnorm_labelled(labels, b, t, Tn)) {
    for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) store4(dx + c, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  float cnt = 0.f;
  for (int tt = 1; tt < Tn; ++tt) cnt += (labels[(int64_t)b * Tn + tt] != -100) ? 1.f : 0.f;
  const float g = 2.f * dloss[0] / ((float)B * fmaxf(cnt, 1e-13f));
#pragma unroll 4
  for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) {
    const float4 v = load4(x + c);
    store4(dx + c, make_float4(g * v.x, g * v.y, g * v.z, g * v.w));
  }
}

}  // namespace mafed

using namespace mafed;

extern "C" int mafed_sqnorm_fwd(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V, float* rowsq,
                                float* out, const int* poison_flag, void* stream) {
  MAFED_CHECK_ARG(logits && labels && rowsq && out, "sqnorm_fwd: null pointer");
  MAFED_CHECK_ARG(B > 0 && T > 0 && V > 0 && V % 4 == 0, "sqnorm_fwd: bad shape (V must be a multiple of 4)");
  hipStream_t st = as_stream(stream);
  dim3 grid((unsigned)((int64_t)B * T)), block(256);
  const double bytes = (double)B * T * V * (dtype == MAFED_F32 ? 4.0 : 2.0);   // the logits, read once (an upper bound: unlabelled rows are skipped)
  if (dtype == MAFED_F32) launch(K_SQNORM, bytes, sqnorm_fwd_kernel<float>, grid, block, 0, st, (const float*)logits, labels, B, T, V, rowsq);
  else launch(K_SQNORM, bytes, sqnorm_fwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)logits, labels, B, T, V, rowsq);
  MAFED_CHECK_LAUNCH("sqnorm_fwd");
  launch(K_SMALL, 0.0, sqnorm_finalize_kernel, dim3(1), block, 0, st, rowsq, labels, B, T, out, poison_flag);
  MAFED_CHECK_LAUNCH("sqnorm_fwd(finalize)");
  return MAFED_OK;
}

extern "C" int mafed_sqnorm_bwd(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V, const float* dloss_dev,
                                void* dlogits, void* stream) {
  MAFED_CHECK_ARG(logits && labels && dloss_dev && dlogits && dlogits != logits, "sqnorm_bwd: null pointer, or dlogits is the logits buffer");
  MAFED_CHECK_ARG(B > 0 && T > 0 && V > 0 && V % 4 == 0, "sqnorm_bwd: bad shape (V must be a multiple of 4)");
  hipStream_t st = as_stream(stream);
  dim3 grid((unsigned)((int64_t)B * T)), block(256);
  const double bytes = 2.0 * B * T * V * (dtype == MAFED_F32 ? 4.0 : 2.0);   // logits in, gradient out
  if (dtype == MAFED_F32) launch(K_SQNORM, bytes, sqnorm_bwd_kernel<float>, grid, block, 0, st, (const float*)logits, labels, B, T, V, dloss_dev, (float*)dlogits);
  else launch(K_SQNORM, bytes, sqnorm_bwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)logits, labels, B, T, V, dloss_dev, (bf16_t*)dlogits);
  MAFED_CHECK_LAUNCH("sqnorm_bwd");
  return MAFED_OK;
}
