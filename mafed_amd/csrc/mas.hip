// Memory Aware Synapses (Aljundi et al. 2018) on the flat fp32 buffers.  State laid out like the parameters:
// importance Omega and anchor p*; the accumulator acc lives only while an importance pass runs.
//   accumulate  (importance pass, per batch)  acc = fma(weight, |g|, acc)                                       8 B read + 4 B written
//   consolidate (between tasks)               Omega = acc / N  (first task)  or  alpha Omega + (1 - alpha) acc / N;  p* = p;  acc = 0
//   penalty     (in front of the clip)        g += 2c Omega (p - p*) in place; leaves the sum-of-squares partials of the g it leaves
//                                             (mafed_gradnorm_finish) and the partials of sum Omega (p - p*)^2    16 B read + 4 B written
// The penalty is SI's stash pass without the stash (penalty_pass.h: one copy of the arithmetic); every scalar stays on the device.
#include "penalty_pass.h"

namespace mafed {

__device__ __forceinline__ float mas_acc1(float g, float a, float w) { return fmaf(w, fabsf(g), a); }

__device__ __forceinline__ float4 mas_acc4(const float* g, const float* acc, int64_t i4, float w) {
  const float4 a = load4(g + i4 * 4), b = load4(acc + i4 * 4);
  return make_float4(mas_acc1(a.x, b.x, w), mas_acc1(a.y, b.y, w), mas_acc1(a.z, b.z, w), mas_acc1(a.w, b.w, w));
}

__global__ __launch_bounds__(256) void mas_accumulate_kernel(const float* __restrict__ g, float* acc, int64_t n, float w) {
  flat_pass2(n,
             [&](int64_t i, int64_t j) {
               const float4 a = mas_acc4(g, acc, i, w), b = mas_acc4(g, acc, j, w);
               store4(acc + i * 4, a);
               store4(acc + j * 4, b);
             },
             [&](int64_t i) { store4(acc + i * 4, mas_acc4(g, acc, i, w)); },
             [&](int64_t t) { acc[t] = mas_acc1(g[t], acc[t], w); });
}

// FIRST: Omega' = k acc with k = 1 / N (Omega is not read: it may hold anything).  Else Omega' = fma(alpha, Omega, k acc) with
// k = (1 - alpha) / N, folded on the host in double: three roundings on the new term (k, k acc, the fma), one on the old.
template <bool FIRST>
__device__ __forceinline__ float mas_cons1(float om, float a, float k, float alpha) { return FIRST ? k * a : fmaf(alpha, om, k * a); }

template <bool FIRST>
__device__ __forceinline__ void mas_cons4(float* acc, float* om, const float* p, float* an, int64_t i4, float k, float alpha) {
  const float4 a = load4(acc + i4 * 4), q = load4(p + i4 * 4);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!FIRST) o = load4(om + i4 * 4);
  store4(om + i4 * 4, make_float4(mas_cons1<FIRST>(o.x, a.x, k, alpha), mas_cons1<FIRST>(o.y, a.y, k, alpha), mas_cons1<FIRST>(o.z, a.z, k, alpha),
                                  mas_cons1<FIRST>(o.w, a.w, k, alpha)));
  store4(an + i4 * 4, q);
  store4(acc + i4 * 4, make_float4(0.f, 0.f, 0.f, 0.f));
}

template <bool FIRST>
__global__ __launch_bounds__(256) void mas_consolidate_kernel(float* __restrict__ acc, float* __restrict__ om, const float* __restrict__ p,
                                                              float* __restrict__ an, int64_t n, float k, float alpha) {
  flat_pass1(n, [&](int64_t i) { mas_cons4<FIRST>(acc, om, p, an, i, k, alpha); },
             [&](int64_t t) {
               om[t] = mas_cons1<FIRST>(FIRST ? 0.f : om[t], acc[t], k, alpha);
               an[t] = p[t];
               acc[t] = 0.f;
             });
}

}  // namespace mafed

using namespace mafed;

extern "C" int mafed_mas_blocks(int64_t n) { return flat_blocks(n, FLAT_BLOCKS_CAP); }

extern "C" int mafed_mas_accumulate(const float* g, float* acc, int64_t n, float weight, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && (n == 0 || (g && acc)), "mas_accumulate: bad arguments");
  MAFED_CHECK_ARG(aligned16({g, acc}), "mas_accumulate: buffers must be 16-byte aligned");
  if (n == 0) return MAFED_OK;
  launch(K_MAS, (double)n * 12.0, mas_accumulate_kernel, dim3((unsigned)mafed_mas_blocks(n)), dim3(256), 0, as_stream(stream), g, acc, n, weight);
  MAFED_CHECK_LAUNCH("mas_accumulate");
  return MAFED_OK;
}

extern "C" int mafed_mas_consolidate(float* acc, float* omega, const float* p, float* anchor, int64_t n, float inv_seen, float alpha, int first,
                                     void* stream) {
  MAFED_CHECK_ARG(n >= 0 && inv_seen > 0.f && alpha >= 0.f && alpha <= 1.f && (n == 0 || (acc && omega && p && anchor)),
                  "mas_consolidate: bad arguments (inv_seen must be positive, alpha in [0, 1])");
  MAFED_CHECK_ARG(aligned16({acc, omega, p, anchor}), "mas_consolidate: buffers must be 16-byte aligned");
  if (n == 0) return MAFED_OK;
  const dim3 grid((unsigned)mafed_mas_blocks(n));
  if (first)
    launch(K_MAS, (double)n * 20.0, mas_consolidate_kernel<true>, grid, dim3(256), 0, as_stream(stream), acc, omega, p, anchor, n, inv_seen, alpha);
  else
    launch(K_MAS, (double)n * 24.0, mas_consolidate_kernel<false>, grid, dim3(256), 0, as_stream(stream), acc, omega, p, anchor, n,
           (float)((1.0 - (double)alpha) * (double)inv_seen), alpha);
  MAFED_CHECK_LAUNCH("mas_consolidate");
  return MAFED_OK;
}

extern "C" int mafed_mas_penalty(float* g, const float* p, const float* omega, const float* anchor, int64_t n, float two_c,
                                 float* sumsq_partials, float* pen_partials, void* stream) {
  MAFED_CHECK_ARG(sumsq_partials && pen_partials && n >= 0 && (n == 0 || (g && p && omega && anchor)), "mas_penalty: bad arguments");
  MAFED_CHECK_ARG(aligned16({g, p, omega, anchor}), "mas_penalty: buffers must be 16-byte aligned");
  const dim3 grid((unsigned)mafed_mas_blocks(n));   // (n == 0: one block that writes a zero partial of each kind)
  launch(K_MAS, (double)n * 20.0, penalty_pass_kernel<true, false>, grid, dim3(256), 0, as_stream(stream), g, p, omega, anchor, n, two_c,
         (float*)nullptr, (float*)nullptr, sumsq_partials, pen_partials);
  MAFED_CHECK_LAUNCH("mas_penalty");
  return MAFED_OK;
}
