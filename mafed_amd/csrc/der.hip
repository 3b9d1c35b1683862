// Dark Experience Replay (DER++) head loss: the shifted, per-sample-normalised cross-entropy of ce.hip plus the
// squared distance between the student's logits s and the logits z the model gave on the same answer token when the sample entered
// the replay memory, in ONE pass per direction:
//   CE  = lse(s) - s[lab]                                                     (ce.hip; mafed/model/vl_pythia.py:86-96)
//   MSE = (1 / V) sum_c (s[c] - z[c])^2
//   loss = beta CE + alpha MSE, both terms summed over a sample's labelled rows / max(count_b, 1e-13), then averaged over B
//   dlogits = g_b (beta (softmax(s) - onehot(lab)) + alpha (2 / V) (s - z)),  g_b = dloss / (B count_b)
// z is read where it is stored: the store is [n_mem, A, V], head row (b, t) reads store[mem_index[b], j, :] with j the rank of the row
// among its sample's labelled rows (HeadRow::rank) -- the same j on the dense and on the row-sparse head, so one kernel serves both and
// no gathered [rows, V] copy of the targets exists.  A labelled row whose sample index is outside [0, n_mem) or whose rank is >= A
// has no stored row: it reads nothing of the store and answers with NaN (row_mse, dlogits), so the step fails loudly.
// HBM-bound like ce.hip and on its column walk: one 256-thread block per head row, 4-element loads (16 bytes fp32, 8 bytes bf16), the
// log-sum-exp through ce.hip's own lse4_step / block_lse -- with z == s and beta == 1 the loss, the saved log-sum-exp and the gradient
// are the cross-entropy kernels' bit for bit.  (kd.hip's 8-element bf16 loads give a thread other columns, hence another rounding of
// the sum: the two cannot be had together.)  Rows without a label are not read at all.  A thread walks its columns in ascending order
// and the block combines in one fixed tree: no atomics, no workspace, the same bits on every call.
#include "head_rows.h"

namespace mafed {

// the stored row of head row `row`, or null where there is none (block-uniform)
template <typename T>
__device__ __forceinline__ const T* anchor_row(const HeadRow& row, const T* store, const int64_t* mem_index, int64_t V, int64_t n_mem, int A) {
  const int64_t m = mem_index[row.b];
  const int j = row.rank();
  if (m < 0 || m >= n_mem || j >= A) return nullptr;
  return store + (m * A + j) * V;
}

// lse, row_ce, row_mse [R]; R = B * Tn.  Unlabelled rows: zeros, nothing read.
template <typename T>
__global__ __launch_bounds__(256) void ce_mse_fwd_kernel(const T* __restrict__ student, const T* __restrict__ store,
                                                         const int64_t* __restrict__ labels, const int64_t* __restrict__ mem_index, int B,
                                                         int Tn, int64_t V, int64_t n_mem, int A, float* __restrict__ lse_out,
                                                         float* __restrict__ row_ce, float* __restrict__ row_mse) {
  __shared__ float sm[8];
  const HeadRow row(labels, Tn);
  const int64_t r = row.r;
  const int64_t lab = row.label();
  if (lab == -100) {   // block-uniform
    if (threadIdx.x == 0) { lse_out[r] = 0.f; row_ce[r] = 0.f; row_mse[r] = 0.f; }
    return;
  }
  const T* xs = student + r * V;
  const T* xz = anchor_row(row, store, mem_index, V, n_mem, A);
  float m = -INFINITY, s = 0.f, q = 0.f;
  if (xz) {
    for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) {
      const float4 v = load4(xs + c), z = load4(xz + c);
      lse4_step(m, s, v);
      const float d0 = v.x - z.x, d1 = v.y - z.y, d2 = v.z - z.z, d3 = v.w - z.w;   // the difference first: exactly 0 where the two agree
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  } else {
    for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) lse4_step(m, s, load4(xs + c));
  }
  const RowLse l = block_lse(m, s, sm);
  q = block_sum<256>(q, sm);
  if (threadIdx.x == 0) {
    const float lse = l.value();
    lse_out[r] = lse;
    row_ce[r] = (lab >= 0 && lab < V) ? (lse - Elem<T>::load(xs + lab)) : 0.f;
    row_mse[r] = xz ? q / (float)V : __int_as_float(0x7fc00000);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_mse_bwd_kernel(const T* __restrict__ student, const T* __restrict__ store,
                                                         const int64_t* __restrict__ labels, const int64_t* __restrict__ mem_index,
                                                         const float* __restrict__ lse, int B, int Tn, int64_t V, int64_t n_mem, int A,
                                                         float alpha2v, float beta, const float* __restrict__ gloss, T* __restrict__ dlogits) {
  const HeadRow row(labels, Tn);
  const int64_t r = row.r;
  T* dx = dlogits + r * V;
  const int64_t lab = row.label();
  if (lab == -100) return zero_row(dx, V);
  const T* xs = student + r * V;
  const T* xz = anchor_row(row, store, mem_index, V, n_mem, A);
  if (!xz) {
    const float nan = __int_as_float(0x7fc00000);
    for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) store4(dx + c, make_float4(nan, nan, nan, nan));
    return;
  }
  const float den = row.denominator(B);
  const float g = gloss[0] / den;
  const float gb = g * beta, ga = g * alpha2v;   // (beta == 1: gb is g, and with z == s what follows is ce_bwd_kernel's arithmetic)
  const float l = lse[r];
  for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) {
    const float4 v = load4(xs + c), z = load4(xz + c);
    float4 o = make_float4(gb * expf(v.x - l) + ga * (v.x - z.x), gb * expf(v.y - l) + ga * (v.y - z.y), gb * expf(v.z - l) + ga * (v.z - z.z),
                           gb * expf(v.w - l) + ga * (v.w - z.w));
    if (lab >= c && lab < c + 4) {   // (no column matches a label outside [0, V))
      const int k = (int)(lab - c);
      if (k == 0) o.x -= gb; else if (k == 1) o.y -= gb; else if (k == 2) o.z -= gb; else o.w -= gb;
    }
    store4(dx + c, o);
  }
}

}  // namespace mafed

using namespace mafed;

static int der_args_check(const void* student, const void* store, const void* dlogits, mafed_dtype dtype, int B, int T, int64_t V,
                          int64_t n_mem, int A, float alpha, float beta, const char* who) {
  MAFED_CHECK_ARG(dtype == MAFED_F32 || dtype == MAFED_BF16, "%s: dtype must be F32 or BF16", who);
  MAFED_HEAD_CHECK_SHAPE(B, T, V, who);
  MAFED_CHECK_ARG(n_mem > 0 && A > 0, "%s: the store must hold at least one sample and one answer row", who);
  MAFED_CHECK_ARG(alpha == alpha && beta == beta && fabsf(alpha) != INFINITY && fabsf(beta) != INFINITY, "%s: alpha and beta must be finite", who);
  // (V % 4 == 0: every row of the three tensors then starts on the boundary its base does)
  const uintptr_t all = (uintptr_t)student | (uintptr_t)store | (uintptr_t)dlogits;
  MAFED_CHECK_ARG((all & 7) == 0, "%s: logits, store and gradient must be 8-byte aligned", who);
  MAFED_CHECK_ARG(dtype == MAFED_BF16 || (all & 15) == 0, "%s: fp32 tensors must be 16-byte aligned", who);
  return MAFED_OK;
}

// out3 = { beta CE + alpha MSE, CE, MSE } (head_finalize_kernel)
extern "C" int mafed_ce_mse_fwd(const void* student, const void* store, mafed_dtype dtype, const int64_t* labels, const int64_t* mem_index,
                                int B, int T, int64_t V, int64_t n_mem, int A, float alpha, float beta, float* lse, float* row_ce,
                                float* row_mse, float* out3, const int* poison_flag, void* stream) {
  MAFED_HEAD_CHECK_PTRS(student && store && labels && mem_index && lse && row_ce && row_mse && out3, "ce_mse_fwd");
  if (der_args_check(student, store, nullptr, dtype, B, T, V, n_mem, A, alpha, beta, "ce_mse_fwd") != MAFED_OK) return MAFED_EINVAL;
  const HeadPass pass(dtype, B, T, V, stream);
  // student logits and the stored rows, each read once
  pass.rows(K_CE_MSE_FWD, 2.0, [](auto e) { return ce_mse_fwd_kernel<decltype(e)>; }, student, store, labels, mem_index, B, T, V, n_mem, A, lse,
            row_ce, row_mse);
  MAFED_CHECK_LAUNCH("ce_mse_fwd");
  pass.finalize<2>(row_ce, row_mse, labels, B, T, alpha, out3, poison_flag, beta);
  MAFED_CHECK_LAUNCH("ce_mse_fwd(finalize)");
  return MAFED_OK;
}

extern "C" int mafed_ce_mse_bwd(const void* student, const void* store, mafed_dtype dtype, const int64_t* labels, const int64_t* mem_index,
                                const float* lse, int B, int T, int64_t V, int64_t n_mem, int A, float alpha, float beta,
                                const float* gloss_dev, void* dlogits, void* stream) {
  MAFED_HEAD_CHECK_PTRS(student && store && labels && mem_index && lse && gloss_dev && dlogits, "ce_mse_bwd");
  if (der_args_check(student, store, dlogits, dtype, B, T, V, n_mem, A, alpha, beta, "ce_mse_bwd") != MAFED_OK) return MAFED_EINVAL;
  const float alpha2v = alpha * (2.0f / (float)V);
  // student logits and the stored rows in, gradient out
  HeadPass(dtype, B, T, V, stream)
      .rows(K_CE_MSE_BWD, 3.0, [](auto e) { return ce_mse_bwd_kernel<decltype(e)>; }, student, store, labels, mem_index, lse, B, T, V, n_mem, A,
            alpha2v, beta, gloss_dev, dlogits);
  MAFED_CHECK_LAUNCH("ce_mse_bwd");
  return MAFED_OK;
}
