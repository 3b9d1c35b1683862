// Squared-norm head objective of the MAS importance pass: J = mean_b( sum_t |z[b,t]|^2 / max(count_b, 1e-13) ) over
// the rows whose shifted label is a token -- the rows and the normaliser of the cross-entropy (ce.hip); the label values are never used.
// HBM-bound: one 256-thread block per (b,t) row, 4-element vector loads, fp32 accumulation; no atomics, the same bits on every call.
#include "head_rows.h"

namespace mafed {

template <typename T>
__global__ __launch_bounds__(256) void sqnorm_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels, int B, int Tn,
                                                         int64_t V, float* __restrict__ rowsq) {
  __shared__ float sm[4];
  const HeadRow row(labels, Tn);
  if (!row.labelled()) {   // every unlabelled row is skipped, not only the last position
    if (threadIdx.x == 0) rowsq[row.r] = 0.f;
    return;
  }
  const T* x = logits + row.r * V;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll 4   // four loads in flight per thread: the sparse head's 256 rows are one block per CU
  for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) {
    const float4 v = load4(x + c);
    s0 += v.x * v.x + v.y * v.y;
    s1 += v.z * v.z + v.w * v.w;
  }
  const float s = block_sum<256>(s0 + s1, sm);
  if (threadIdx.x == 0) rowsq[row.r] = s;
}

// dJ/dz = 2 z dloss / (B max(count_b, 1e-13)) on labelled rows, zeros elsewhere; dlogits is a buffer of its own
template <typename T>
__global__ __launch_bounds__(256) void sqnorm_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels, int B, int Tn, int64_t V,
                                                         const float* __restrict__ dloss, T* __restrict__ dlogits) {
  const HeadRow row(labels, Tn);
  const T* x = logits + row.r * V;
  T* dx = dlogits + row.r * V;
  if (!row.labelled()) return zero_row(dx, V);
  const float den = row.denominator(B);
  const float g = 2.f * dloss[0] / den;   // (2 dloss) / den
#pragma unroll 4
  for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) {
    const float4 v = load4(x + c);
    store4(dx + c, make_float4(g * v.x, g * v.y, g * v.z, g * v.w));
  }
}

}  // namespace mafed

using namespace mafed;

// out = mean_b( sum_t rowsq[b,t] / max(count_b, 1e-13) ) (head_finalize_kernel)
extern "C" int mafed_sqnorm_fwd(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V, float* rowsq,
                                float* out, const int* poison_flag, void* stream) {
  MAFED_HEAD_CHECK_PTRS(logits && labels && rowsq && out, "sqnorm_fwd");
  MAFED_HEAD_CHECK_SHAPE(B, T, V, "sqnorm_fwd");
  const HeadPass pass(dtype, B, T, V, stream);
  // the logits, read once (an upper bound: unlabelled rows are skipped)
  pass.rows(K_SQNORM, 1.0, [](auto e) { return sqnorm_fwd_kernel<decltype(e)>; }, logits, labels, B, T, V, rowsq);
  MAFED_CHECK_LAUNCH("sqnorm_fwd");
  pass.finalize<1>(rowsq, nullptr, labels, B, T, 0.f, out, poison_flag);
  MAFED_CHECK_LAUNCH("sqnorm_fwd(finalize)");
  return MAFED_OK;
}

extern "C" int mafed_sqnorm_bwd(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V, const float* dloss_dev,
                                void* dlogits, void* stream) {
  MAFED_CHECK_ARG(logits && labels && dloss_dev && dlogits && dlogits != logits, "sqnorm_bwd: null pointer, or dlogits is the logits buffer");
  MAFED_HEAD_CHECK_SHAPE(B, T, V, "sqnorm_bwd");
  // logits in, gradient out
  HeadPass(dtype, B, T, V, stream).rows(K_SQNORM, 2.0, [](auto e) { return sqnorm_bwd_kernel<decltype(e)>; }, logits, labels, B, T, V, dloss_dev, dlogits);
  MAFED_CHECK_LAUNCH("sqnorm_bwd");
  return MAFED_OK;
}
