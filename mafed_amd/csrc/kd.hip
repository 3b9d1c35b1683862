// Learning without Forgetting head loss: the shifted, per-sample-normalised cross-entropy of ce.hip plus a
// temperature-softened KL term between a frozen teacher's logits t and the student's logits s of the same head rows, in ONE pass per
// direction:
//   CE  = lse(s) - s[lab]                                                     (ce.hip; mafed/model/vl_pythia.py:86-96)
//   KD  = KL(softmax(t / tau) || softmax(s / tau)) = sum_c p_t[c] (t[c] - s[c]) / tau - lse(t / tau) + lse(s / tau)
//   loss = CE + lambda tau^2 KD, both terms summed over a sample's labelled rows / max(count_b, 1e-13), then averaged over B
//   dlogits = g_b (softmax(s) - onehot(lab)) + g_b lambda tau (softmax(s / tau) - softmax(t / tau)),  g_b = dloss / (B count_b)
// HBM-bound like ce.hip: one 256-thread block per head row, 16-byte loads (4 fp32 / 8 bf16 elements; 8-byte bf16 loads when V % 8 != 0),
// every accumulator an online, max-subtracted fp32 one.  Rows without a label (ignore_index, the last position) are not read at all.
// A thread walks its columns in ascending order and the block combines the partials in one fixed tree: no atomics, no workspace, the
// same bits on every call.
#include "head_rows.h"

namespace mafed {

template <typename T, int VEC>
struct RowVec;
template <typename T>
struct RowVec<T, 4> {   // load4 / store4 of common.h
  static __device__ __forceinline__ void load(const T* p, float (&v)[4]) {
    const float4 r = load4(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  }
  static __device__ __forceinline__ void store(T* p, const float (&v)[4]) { store4(p, make_float4(v[0], v[1], v[2], v[3])); }
};
template <>
struct RowVec<bf16_t, 8> {
  static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] = __uint_as_float(w[k] << 16); v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u); }
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (uint32_t)f32_to_bf16(v[2 * k]) | ((uint32_t)f32_to_bf16(v[2 * k + 1]) << 16);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

template <int VEC>
__device__ __forceinline__ float tree_sum(const float (&e)[VEC]) {
  static_assert(VEC == 4 || VEC == 8, "4 or 8 elements per load");
  if constexpr (VEC == 4) return (e[0] + e[1]) + (e[2] + e[3]);
  else return ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
}

// One step of an online log-sum-exp over VEC arguments: (m, s) <- running max / sum of exp(a - m); e[k] = exp(a[k] - m) under the new max.
// Returns the factor the old sum was rescaled by (1 when the max did not move): a second sum weighted by e follows it (the teacher-weighted
// difference).  The three accumulators of a row all go through this one function, contraction off: equal arguments give equal bits --
// tau == 1 makes the two student LSEs the same number, student == teacher makes the two tau-domain LSEs the same number.
template <int VEC>
__device__ __forceinline__ float online_step(float& m, float& s, const float (&a)[VEC], float (&e)[VEC]) {
#pragma clang fp contract(off)
  float mx = a[0];
#pragma unroll
  for (int k = 1; k < VEC; ++k) mx = fmaxf(mx, a[k]);
  float f = 1.f;
  if (mx > m) { f = __expf(m - mx); s = s * f; m = mx; }
#pragma unroll
  for (int k = 0; k < VEC; ++k) e[k] = __expf(a[k] - m);
  s = s + tree_sum<VEC>(e);
  return f;
}

// block combine of one online accumulator: per-wave max, rescale, per-wave sum (lane 0 of each wave then holds (gm, gs[, gd]))
__device__ __forceinline__ void wave_combine(float& m, float& s, float* d) {
#pragma clang fp contract(off)
  const float gm = wave_max(m);
  const float f = (m == -INFINITY) ? 0.f : __expf(m - gm);   // (a thread that saw no column: its empty sums stay out)
  s = wave_sum(s * f);
  if (d) *d = wave_sum(*d * f);
  m = gm;
}

// sm: [4 waves][8] = {m1, s1, m2, s2, m3, s3, d, -}; thread 0 folds the four waves in fixed order
__device__ __forceinline__ void fold_waves(const float* sm, int im, int is, int id, float& M, float& S, float* D) {
#pragma clang fp contract(off)
  M = fmaxf(fmaxf(sm[im], sm[8 + im]), fmaxf(sm[16 + im], sm[24 + im]));
  float f[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) f[w] = (sm[8 * w + im] == -INFINITY) ? 0.f : __expf(sm[8 * w + im] - M);
  S = (sm[is] * f[0] + sm[8 + is] * f[1]) + (sm[16 + is] * f[2] + sm[24 + is] * f[3]);
  if (D) *D = (sm[id] * f[0] + sm[8 + id] * f[1]) + (sm[16 + id] * f[2] + sm[24 + id] * f[3]);
}

// lse3 [3, R] = { lse(s), lse(s / tau), lse(t / tau) }, row_ce / row_kd [R]; R = B * Tn.  Unlabelled rows: zeros, nothing read.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void ce_kd_fwd_kernel(const T* __restrict__ student, const T* __restrict__ teacher,
                                                        const int64_t* __restrict__ labels, int B, int Tn, int64_t V, float inv_tau,
                                                        float* __restrict__ lse3, float* __restrict__ row_ce, float* __restrict__ row_kd) {
  __shared__ float sm[32];
  const HeadRow row(labels, Tn);
  const int64_t r = row.r, R = (int64_t)B * Tn;
  const int64_t lab = row.label();
  if (lab == -100) {   // block-uniform
    if (threadIdx.x == 0) { lse3[r] = 0.f; lse3[R + r] = 0.f; lse3[2 * R + r] = 0.f; row_ce[r] = 0.f; row_kd[r] = 0.f; }
    return;
  }
  const T* xs = student + r * V;
  const T* xt = teacher + r * V;
  float m1 = -INFINITY, s1 = 0.f, m2 = -INFINITY, s2 = 0.f, m3 = -INFINITY, s3 = 0.f, d = 0.f;
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < V; c += 256 * VEC) {
    float sv[VEC], tv[VEC], as[VEC], at[VEC], e[VEC], w[VEC];
    RowVec<T, VEC>::load(xs + c, sv);
    RowVec<T, VEC>::load(xt + c, tv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      as[k] = __fmul_rn(sv[k], inv_tau);
      at[k] = __fmul_rn(tv[k], inv_tau);
    }
    online_step<VEC>(m1, s1, sv, e);
    online_step<VEC>(m2, s2, as, e);
    const float f = online_step<VEC>(m3, s3, at, e);
#pragma unroll
    for (int k = 0; k < VEC; ++k) w[k] = e[k] * ((tv[k] - sv[k]) * inv_tau);   // from (t - s): exactly 0 where the two agree
    d = d * f + tree_sum<VEC>(w);
  }
  wave_combine(m1, s1, nullptr);
  wave_combine(m2, s2, nullptr);
  wave_combine(m3, s3, &d);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    float* o = sm + 8 * wave;
    o[0] = m1; o[1] = s1; o[2] = m2; o[3] = s2; o[4] = m3; o[5] = s3; o[6] = d;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M1, S1, M2, S2, M3, S3, D;
    fold_waves(sm, 0, 1, 0, M1, S1, nullptr);
    fold_waves(sm, 2, 3, 0, M2, S2, nullptr);
    fold_waves(sm, 4, 5, 6, M3, S3, &D);
    const float l1 = M1 + logf(S1), l2 = M2 + logf(S2), l3 = M3 + logf(S3);
    lse3[r] = l1; lse3[R + r] = l2; lse3[2 * R + r] = l3;
    row_ce[r] = (lab >= 0 && lab < V) ? (l1 - Elem<T>::load(xs + lab)) : 0.f;
    row_kd[r] = (D / S3 - l3) + l2;   // student == teacher: D = 0 and l2, l3 the same bits -> exactly 0
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void ce_kd_bwd_kernel(const T* __restrict__ student, const T* __restrict__ teacher,
                                                        const int64_t* __restrict__ labels, const float* __restrict__ lse3, int B, int Tn,
                                                        int64_t V, float inv_tau, float lam_tau, const float* __restrict__ gloss,
                                                        T* __restrict__ dlogits) {
  const HeadRow row(labels, Tn);
  const int64_t r = row.r, R = (int64_t)B * Tn;
  T* dx = dlogits + r * V;
  const int64_t lab = row.label();
  if (lab == -100) return zero_row<T, VEC>(dx, V);
  const T* xs = student + r * V;
  const T* xt = teacher + r * V;
  const float den = row.denominator(B);
  const float g = gloss[0] / den;
  const float gk = g * lam_tau;
  const float l1 = lse3[r], l2 = lse3[R + r], l3 = lse3[2 * R + r];
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < V; c += 256 * VEC) {
    float sv[VEC], tv[VEC], o[VEC];
    RowVec<T, VEC>::load(xs + c, sv);
    RowVec<T, VEC>::load(xt + c, tv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      // (the two tau-domain probabilities by the same instructions: student == teacher leaves the cross-entropy gradient alone)
      const float ps = __expf(__fmul_rn(sv[k], inv_tau) - l2), pt = __expf(__fmul_rn(tv[k], inv_tau) - l3);
      o[k] = g * __expf(sv[k] - l1) + gk * (ps - pt);
      if (c + k == lab) o[k] -= g;
    }
    RowVec<T, VEC>::store(dx + c, o);
  }
}

}  // namespace mafed

using namespace mafed;

static int kd_args_check(const void* student, const void* teacher, int B, int T, int64_t V, float tau, float lambda, const char* who) {
  MAFED_HEAD_CHECK_SHAPE(B, T, V, who);
  MAFED_CHECK_ARG(tau > 0.f && tau < INFINITY && lambda == lambda && fabsf(lambda) != INFINITY, "%s: tau must be positive and finite, lambda finite", who);
  MAFED_CHECK_ARG(((((uintptr_t)student) | ((uintptr_t)teacher)) & 7) == 0, "%s: logits must be 8-byte aligned", who);
  return MAFED_OK;
}

// 8 bf16 elements per load when every row of both matrices (and of the gradient) starts on a 16-byte boundary
static bool kd_wide(mafed_dtype dtype, int64_t V, const void* a, const void* b, const void* c) {
  return dtype == MAFED_BF16 && V % 8 == 0 && ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0;
}

// out3 = { CE + lambda tau^2 KD, CE, KD } (head_finalize_kernel)
extern "C" int mafed_ce_kd_fwd(const void* student, const void* teacher, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V,
                               float tau, float lambda, float* lse3, float* row_ce, float* row_kd, float* out3, const int* poison_flag,
                               void* stream) {
  MAFED_HEAD_CHECK_PTRS(student && teacher && labels && lse3 && row_ce && row_kd && out3, "ce_kd_fwd");
  MAFED_CHECK_ARG(dtype == MAFED_F32 || dtype == MAFED_BF16, "ce_kd_fwd: dtype must be F32 or BF16");
  if (kd_args_check(student, teacher, B, T, V, tau, lambda, "ce_kd_fwd") != MAFED_OK) return MAFED_EINVAL;
  MAFED_CHECK_ARG(dtype == MAFED_BF16 || (((uintptr_t)student | (uintptr_t)teacher) & 15) == 0, "ce_kd_fwd: fp32 logits must be 16-byte aligned");
  const HeadPass pass(dtype, B, T, V, stream);
  const bool wide = kd_wide(dtype, V, student, teacher, nullptr);
  const float inv_tau = 1.0f / tau;
  // student and teacher logits, each read once
  pass.rows(K_CE_KD_FWD, 2.0, [wide](auto e) { using E = decltype(e); return wide ? ce_kd_fwd_kernel<E, 16 / sizeof(E)> : ce_kd_fwd_kernel<E, 4>; },
            student, teacher, labels, B, T, V, inv_tau, lse3, row_ce, row_kd);
  MAFED_CHECK_LAUNCH("ce_kd_fwd");
  pass.finalize<2>(row_ce, row_kd, labels, B, T, lambda * tau * tau, out3, poison_flag);
  MAFED_CHECK_LAUNCH("ce_kd_fwd(finalize)");
  return MAFED_OK;
}

extern "C" int mafed_ce_kd_bwd(const void* student, const void* teacher, mafed_dtype dtype, const int64_t* labels, const float* lse3, int B,
                               int T, int64_t V, float tau, float lambda, const float* gloss_dev, void* dlogits, void* stream) {
  MAFED_HEAD_CHECK_PTRS(student && teacher && labels && lse3 && gloss_dev && dlogits, "ce_kd_bwd");
  MAFED_CHECK_ARG(dtype == MAFED_F32 || dtype == MAFED_BF16, "ce_kd_bwd: dtype must be F32 or BF16");
  if (kd_args_check(student, teacher, B, T, V, tau, lambda, "ce_kd_bwd") != MAFED_OK) return MAFED_EINVAL;
  MAFED_CHECK_ARG((((uintptr_t)dlogits) & 7) == 0, "ce_kd_bwd: dlogits must be 8-byte aligned");
  MAFED_CHECK_ARG(dtype == MAFED_BF16 || (((uintptr_t)student | (uintptr_t)teacher | (uintptr_t)dlogits) & 15) == 0,
                  "ce_kd_bwd: fp32 tensors must be 16-byte aligned");
  const bool wide = kd_wide(dtype, V, student, teacher, dlogits);
  const float inv_tau = 1.0f / tau, lam_tau = lambda * tau;
  // student and teacher logits in, gradient out
  HeadPass(dtype, B, T, V, stream)
      .rows(K_CE_KD_BWD, 3.0, [wide](auto e) { using E = decltype(e); return wide ? ce_kd_bwd_kernel<E, 16 / sizeof(E)> : ce_kd_bwd_kernel<E, 4>; },
            student, teacher, labels, lse3, B, T, V, inv_tau, lam_tau, gloss_dev, dlogits);
  MAFED_CHECK_LAUNCH("ce_kd_bwd");
  return MAFED_OK;
}
