// Shifted, per-sample-normalised cross-entropy over the text positions (mafed/model/vl_pythia.py:44-96).
// HBM-bound: one 256-thread block per (b,t) row, 4-element vector loads, online log-sum-exp in fp32.
#include "head_rows.h"

namespace mafed {

template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels, int B, int Tn,
                                                     int64_t V, float* __restrict__ lse_out, float* __restrict__ row_loss) {
  __shared__ float sm[8];
  const HeadRow row(labels, Tn);
  const int64_t r = row.r;
  if (row.last()) {  // only the last position is skipped: a row whose label is the ignore index still gets its lse (ops.ce_fwd returns it)
    if (threadIdx.x == 0) { row_loss[r] = 0.f; lse_out[r] = 0.f; }
    return;
  }
  const T* x = logits + r * V;
  const RowLse l = row_lse4(x, V, sm);
  if (threadIdx.x == 0) {
    const float lse = l.value();
    lse_out[r] = lse;
    const int64_t lab = row.next_label();
    // ignore_index -100 -> 0, and so does a label outside [0, V): that row still counts in the normaliser
    row_loss[r] = (lab >= 0 && lab < V) ? (lse - Elem<T>::load(x + lab)) : 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ lse, int B, int Tn, int64_t V,
                                                     const float* __restrict__ gloss, T* __restrict__ dlogits) {
  const HeadRow row(labels, Tn);
  const int64_t r = row.r;
  const T* x = logits + r * V;
  T* dx = dlogits + r * V;
  const int64_t lab = row.label();
  if (lab == -100) return zero_row(dx, V);
  const float den = row.denominator(B);
  const float g = gloss[0] / den;
  const float l = lse[r];
  for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) {
    const float4 v = load4(x + c);
    float4 o = make_float4(g * expf(v.x - l), g * expf(v.y - l), g * expf(v.z - l), g * expf(v.w - l));
    if (lab >= c && lab < c + 4) {   // (no column matches a label outside [0, V))
      const int k = (int)(lab - c);
      if (k == 0) o.x -= g; else if (k == 1) o.y -= g; else if (k == 2) o.z -= g; else o.w -= g;
    }
    store4(dx + c, o);
  }
}

}  // namespace mafed

using namespace mafed;

// loss = mean_b( sum_t row_loss[b,t] / max(count_b, 1e-13) ) (head_finalize_kernel)
static int ce_fwd_impl(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V, float* lse, float* row_loss,
                       float* loss_out, const int* poison, void* stream) {
  MAFED_HEAD_CHECK_PTRS(logits && labels && lse && row_loss && loss_out, "ce_fwd");
  MAFED_HEAD_CHECK_SHAPE(B, T, V, "ce_fwd");
  const HeadPass pass(dtype, B, T, V, stream);
  pass.rows(K_CE_FWD, 1.0, [](auto e) { return ce_fwd_kernel<decltype(e)>; }, logits, labels, B, T, V, lse, row_loss);  // the logits, read once
  MAFED_CHECK_LAUNCH("ce_fwd");
  pass.finalize<1>(row_loss, nullptr, labels, B, T, 0.f, loss_out, poison);
  MAFED_CHECK_LAUNCH("ce_fwd(finalize)");
  return MAFED_OK;
}

extern "C" int mafed_ce_fwd(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V, float* lse,
                            float* row_loss, float* loss_out, void* stream) {
  return ce_fwd_impl(logits, dtype, labels, B, T, V, lse, row_loss, loss_out, nullptr, stream);
}

extern "C" int mafed_ce_fwd_guarded(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V, float* lse,
                                    float* row_loss, float* loss_out, const int* poison_flag, void* stream) {
  MAFED_CHECK_ARG(poison_flag, "ce_fwd_guarded: null flag");
  return ce_fwd_impl(logits, dtype, labels, B, T, V, lse, row_loss, loss_out, poison_flag, stream);
}

extern "C" int mafed_ce_bwd(const void* logits, mafed_dtype dtype, const int64_t* labels, const float* lse, int B, int T, int64_t V,
                            const float* gloss_dev, void* dlogits, void* stream) {
  MAFED_HEAD_CHECK_PTRS(logits && labels && lse && gloss_dev && dlogits, "ce_bwd");
  MAFED_HEAD_CHECK_SHAPE(B, T, V, "ce_bwd");
  HeadPass(dtype, B, T, V, stream).rows(K_CE_BWD, 2.0, [](auto e) { return ce_bwd_kernel<decltype(e)>; }, logits, labels, lse, B, T, V, gloss_dev, dlogits);  // logits in, gradient out
  MAFED_CHECK_LAUNCH("ce_bwd");
  return MAFED_OK;
}
