// Log-probability of GIVEN tokens (model.score; DESIGN.md section 4c''''): out[r] = logits[row(r), target[r]] - logsumexp(logits[row(r), :]),
// the per-token term of the reference's shifted cross-entropy (mafed/model/vl_pythia.py:64-96) with the sign turned, and the per-candidate
// sum / mean of those terms.  HBM-bound like ce.hip, whose row reduction this is (head_rows.h: row_lse4): one 256-thread block per
// output row, 4-element vector loads, online log-sum-exp in fp32.  Each thread walks its columns in ascending order and the block combines
// the 256 partial results in one fixed tree, so a row's result is the same bits on every call and does not depend on R or on the other rows.
#include "head_rows.h"

namespace mafed {

// VEC: V % 4 == 0 and every row starts on a 4-element boundary (base pointer and ldl): 16-byte fp32 / 8-byte bf16 loads
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void token_logprob_kernel(const T* __restrict__ logits, int64_t ldl, const int* __restrict__ logits_row,
                                                            const int64_t* __restrict__ target, int64_t V, float* __restrict__ out) {
  __shared__ float sm[8];
  const int64_t r = blockIdx.x;
  const int64_t tgt = target[r];
  if (tgt < 0 || tgt >= V) {  // block-uniform.  < 0: a masked position; >= V: no such token, NaN rather than a read past the row
    if (threadIdx.x == 0) out[r] = tgt < 0 ? 0.f : __int_as_float(0x7fc00000);
    return;
  }
  const T* x = logits + (logits_row ? (int64_t)logits_row[r] : r) * ldl;
  RowLse l;
  if (VEC) {
    l = row_lse4(x, V, sm);
  } else {
    float m = -INFINITY, s = 0.f;
    for (int64_t c = threadIdx.x; c < V; c += 256) {
      const float v = Elem<T>::load(x + c);
      if (v > m) { s *= expf(m - v); m = v; }
      s += expf(v - m);
    }
    l = block_lse(m, s, sm);
  }
  if (threadIdx.x == 0) out[r] = Elem<T>::load(x + tgt) - l.value();
}

// score[r] = sum_j mask[r, j] * tlp[r, j] in ascending j (mean: divided by the count); no token -> -inf.  One thread per candidate.
__global__ __launch_bounds__(256) void score_reduce_kernel(const float* __restrict__ tlp, const int64_t* __restrict__ mask, int R, int A, int mean,
                                                           float* __restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float s = 0.f;
  int n = 0;
  for (int j = 0; j < A; ++j)
    if (!mask || mask[(int64_t)r * A + j] != 0) { s += tlp[(int64_t)r * A + j]; ++n; }
  out[r] = n == 0 ? -INFINITY : (mean ? s / (float)n : s);
}

}  // namespace mafed

using namespace mafed;

extern "C" int mafed_token_logprob(const void* logits, mafed_dtype dtype, int64_t ldl, const int* logits_row, const int64_t* target, int R,
                                   int64_t V, float* out, void* stream) {
  MAFED_CHECK_ARG(logits && target && out, "token_logprob: null pointer");
  MAFED_CHECK_ARG(R > 0 && V > 0 && ldl >= V, "token_logprob: bad shape R=%d V=%lld ldl=%lld", R, (long long)V, (long long)ldl);
  hipStream_t st = as_stream(stream);
  dim3 grid((unsigned)R), block(256);
  const bool f32 = dtype == MAFED_F32;
  const bool vec = V % 4 == 0 && ldl % 4 == 0 && ((uintptr_t)logits & (f32 ? 15 : 7)) == 0;
  const double bytes = (double)R * V * (f32 ? 4.0 : 2.0);  // the logits rows, read once
  if (f32 && vec) launch(K_CE_FWD, bytes, token_logprob_kernel<float, true>, grid, block, 0, st, (const float*)logits, ldl, logits_row, target, V, out);
  else if (f32) launch(K_CE_FWD, bytes, token_logprob_kernel<float, false>, grid, block, 0, st, (const float*)logits, ldl, logits_row, target, V, out);
  else if (vec) launch(K_CE_FWD, bytes, token_logprob_kernel<bf16_t, true>, grid, block, 0, st, (const bf16_t*)logits, ldl, logits_row, target, V, out);
  else launch(K_CE_FWD, bytes, token_logprob_kernel<bf16_t, false>, grid, block, 0, st, (const bf16_t*)logits, ldl, logits_row, target, V, out);
  MAFED_CHECK_LAUNCH("token_logprob");
  return MAFED_OK;
}

extern "C" int mafed_score_reduce(const float* token_logprob, const int64_t* mask, int R, int A, int mean, float* out, void* stream) {
  MAFED_CHECK_ARG(token_logprob && out, "score_reduce: null pointer");
  MAFED_CHECK_ARG(R > 0 && A > 0, "score_reduce: bad shape R=%d A=%d", R, A);
  launch(K_SMALL, 0.0, score_reduce_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, as_stream(stream), token_logprob, mask, R, A, mean, out);
  MAFED_CHECK_LAUNCH("score_reduce");
  return MAFED_OK;
}
