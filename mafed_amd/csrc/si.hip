// Synaptic Intelligence (Zenke, Poole, Ganguli 2017) on the flat fp32 buffers.  State laid out like the
// parameters: path integral w, importance Omega, anchor p*, and the stash pair (g^, p^) of the window that is being stepped.
//   stash       (in front of the clip)   g^ = g   p^ = p   from task 1 on  g += 2c Omega (p - p*)  in place; leaves the sum-of-squares
//                                        partials of the g it leaves (mafed_gradnorm_finish) and the partials of sum Omega (p - p*)^2
//   accumulate  (behind the optimiser)   w -= g^ (p - p^)  where p != p^; an element that did not move keeps its w bit for bit
//   consolidate (between tasks)          Omega = max(Omega + w / ((p - p*)^2 + xi), 0)   p* = p   w = 0
// HBM-bound passes of 16 (task 0), 28, 20 and 28 bytes per parameter; the penalty never enters autograd and every scalar stays on the
// device.
#include "penalty_pass.h"   // the stash pass is penalty_pass_kernel<PEN, STASH = true>, shared with mas.hip

namespace mafed {

// One block: the penalty partials folded in double (index order per thread, then a fixed tree) -> out[0] = c * sum
__global__ __launch_bounds__(256) void si_penalty_finish_kernel(const float* __restrict__ partial, int nblk, float c, float* __restrict__ out) {
  __shared__ double sm[256];
  double mine[1];
  fold_partials_f64(partial, nblk, mine);
  const double e = block_sum_f64(mine[0], sm);
  if (threadIdx.x == 0) out[0] = (float)((double)c * e);
}

// w' = w - g^ (p - p^) where the parameter moved; a select, not a multiply by zero: an unmoved element keeps its w whatever g^ holds
// (the step the non-finite-norm guard skipped moved nothing and has a non-finite g^).
__device__ __forceinline__ float si_acc1(float w, float sg, float sp, float p) { return p == sp ? w : fmaf(-sg, p - sp, w); }

__device__ __forceinline__ float4 si_acc4(const float* sg, const float* sp, const float* p, const float* w, int64_t i4) {
  const float4 a = load4(sg + i4 * 4), b = load4(sp + i4 * 4), c = load4(p + i4 * 4), d = load4(w + i4 * 4);
  return make_float4(si_acc1(d.x, a.x, b.x, c.x), si_acc1(d.y, a.y, b.y, c.y), si_acc1(d.z, a.z, b.z, c.z), si_acc1(d.w, a.w, b.w, c.w));
}

__global__ __launch_bounds__(256) void si_accumulate_kernel(const float* __restrict__ sg, const float* __restrict__ sp,
                                                            const float* __restrict__ p, float* w, int64_t n) {
  flat_pass2(n,
             [&](int64_t i, int64_t j) {
               const float4 a = si_acc4(sg, sp, p, w, i), b = si_acc4(sg, sp, p, w, j);
               store4(w + i * 4, a);
               store4(w + j * 4, b);
             },
             [&](int64_t i) { store4(w + i * 4, si_acc4(sg, sp, p, w, i)); },
             [&](int64_t t) { w[t] = si_acc1(w[t], sg[t], sp[t], p[t]); });
}

// Omega' = max(Omega + w / ((p - p*)^2 + xi), 0): a true division; a negative sum gives exactly +0, a NaN stays a NaN
__device__ __forceinline__ float si_cons1(float om, float w, float p, float an, float xi) {
  const float d = p - an;
  const float v = om + w / fmaf(d, d, xi);
  return v < 0.f ? 0.f : v;
}

__device__ __forceinline__ void si_cons4(const float* p, float* an, float* w, float* om, int64_t i4, float xi) {
  const float4 a = load4(p + i4 * 4), q = load4(an + i4 * 4), x = load4(w + i4 * 4), o = load4(om + i4 * 4);
  store4(om + i4 * 4, make_float4(si_cons1(o.x, x.x, a.x, q.x, xi), si_cons1(o.y, x.y, a.y, q.y, xi), si_cons1(o.z, x.z, a.z, q.z, xi),
                                  si_cons1(o.w, x.w, a.w, q.w, xi)));
  store4(an + i4 * 4, a);
  store4(w + i4 * 4, make_float4(0.f, 0.f, 0.f, 0.f));
}

__global__ __launch_bounds__(256) void si_consolidate_kernel(const float* __restrict__ p, float* __restrict__ an, float* __restrict__ w,
                                                             float* __restrict__ om, int64_t n, float xi) {
  flat_pass1(n, [&](int64_t i) { si_cons4(p, an, w, om, i, xi); },
             [&](int64_t t) {
               om[t] = si_cons1(om[t], w[t], p[t], an[t], xi);
               an[t] = p[t];
               w[t] = 0.f;
             });
}

}  // namespace mafed

using namespace mafed;

extern "C" int mafed_si_blocks(int64_t n) { return flat_blocks(n, FLAT_BLOCKS_CAP); }

extern "C" int mafed_si_stash(float* g, const float* p, const float* omega, const float* anchor, int64_t n, float two_c, float* stash_g,
                              float* stash_p, float* sumsq_partials, float* pen_partials, void* stream) {
  MAFED_CHECK_ARG(sumsq_partials && pen_partials && n >= 0 && (n == 0 || (g && p && stash_g && stash_p)), "si_stash: bad arguments");
  MAFED_CHECK_ARG((omega == nullptr) == (anchor == nullptr), "si_stash: omega and anchor come together");
  MAFED_CHECK_ARG(aligned16({g, p, omega, anchor, stash_g, stash_p}), "si_stash: buffers must be 16-byte aligned");
  const dim3 grid((unsigned)mafed_si_blocks(n));   // (n == 0: one block that writes a zero partial of each kind)
  if (omega)
    launch(K_SI, (double)n * 28.0, penalty_pass_kernel<true, true>, grid, dim3(256), 0, as_stream(stream), g, p, omega, anchor, n, two_c, stash_g, stash_p,
           sumsq_partials, pen_partials);
  else
    launch(K_SI, (double)n * 16.0, penalty_pass_kernel<false, true>, grid, dim3(256), 0, as_stream(stream), g, p, omega, anchor, n, two_c, stash_g, stash_p,
           sumsq_partials, pen_partials);
  MAFED_CHECK_LAUNCH("si_stash");
  return MAFED_OK;
}

extern "C" int mafed_si_penalty_finish(const float* pen_partials, int n_partials, float c, float* out, void* stream) {
  MAFED_CHECK_ARG(pen_partials && out && n_partials >= 0, "si_penalty_finish: bad arguments");
  launch(K_SMALL, 0.0, si_penalty_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), pen_partials, n_partials, c, out);
  MAFED_CHECK_LAUNCH("si_penalty_finish");
  return MAFED_OK;
}

extern "C" int mafed_si_accumulate(const float* stash_g, const float* stash_p, const float* p, float* w, int64_t n, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && (n == 0 || (stash_g && stash_p && p && w)), "si_accumulate: bad arguments");
  MAFED_CHECK_ARG(aligned16({stash_g, stash_p, p, w}), "si_accumulate: buffers must be 16-byte aligned");
  if (n == 0) return MAFED_OK;
  launch(K_SI, (double)n * 20.0, si_accumulate_kernel, dim3((unsigned)mafed_si_blocks(n)), dim3(256), 0, as_stream(stream), stash_g, stash_p, p, w, n);
  MAFED_CHECK_LAUNCH("si_accumulate");
  return MAFED_OK;
}

extern "C" int mafed_si_consolidate(const float* p, float* anchor, float* w, float* omega, int64_t n, float xi, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && xi > 0.f && (n == 0 || (p && anchor && w && omega)), "si_consolidate: bad arguments (xi must be positive)");
  MAFED_CHECK_ARG(aligned16({p, anchor, w, omega}), "si_consolidate: buffers must be 16-byte aligned");
  if (n == 0) return MAFED_OK;
  launch(K_SI, (double)n * 28.0, si_consolidate_kernel, dim3((unsigned)mafed_si_blocks(n)), dim3(256), 0, as_stream(stream), p, anchor, w, omega, n, xi);
  MAFED_CHECK_LAUNCH("si_consolidate");
  return MAFED_OK;
}
