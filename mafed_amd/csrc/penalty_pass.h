// The penalty pass that SI's stash (si.hip) and MAS's penalty (mas.hip) share: one read-modify-write of the gradient buffer in front of the
// clip,  g' = g + 2c Omega (p - p*),  that leaves the sum-of-squares partials of g' and the partials of sum Omega (p - p*)^2.  STASH adds
// SI's bit copies g^ = g, p^ = p; without PEN (SI on task 0) g is only read.  One copy of the arithmetic: both methods get the same bits.
#pragma once
#include "flat_pass.h"

namespace mafed {

// One element of the penalty form: d = p - p*, t = Omega d, g' = fma(2c, t, g); pen += t d  (= Omega d^2)
__device__ __forceinline__ float penalty1(float g, float p, float om, float an, float two_c, float& pen) {
  const float d = p - an, t = om * d;
  pen += t * d;
  return fmaf(two_c, t, g);
}

// One vector of the pass.  PEN = false: g is only read.  Every element is read and written by the same thread, all reads of a
// trip in front of its writes -- hence no __restrict__ on g.
template <bool PEN, bool STASH>
__device__ __forceinline__ float4 penalty_pass4(float* g, const float* p, const float* om, const float* an, float* sg, float* sp, int64_t i4,
                                            float two_c, float& pen) {
  float4 a = load4(g + i4 * 4);
  const float4 b = load4(p + i4 * 4);
  if (STASH) {
    store4(sg + i4 * 4, a);
    store4(sp + i4 * 4, b);
  }
  if (PEN) {
    const float4 o = load4(om + i4 * 4), q = load4(an + i4 * 4);
    float p0 = 0.f, p1 = 0.f;
    a.x = penalty1(a.x, b.x, o.x, q.x, two_c, p0);
    a.y = penalty1(a.y, b.y, o.y, q.y, two_c, p1);
    a.z = penalty1(a.z, b.z, o.z, q.z, two_c, p0);
    a.w = penalty1(a.w, b.w, o.w, q.w, two_c, p1);
    pen += p0 + p1;
    store4(g + i4 * 4, a);
  }
  return a;
}

// sumsq[b], pen_out[b] = this block's shares of sum g'^2 and sum Omega (p - p*)^2: the vectors of a pair into (s0, e0) and (s1, e1),
// a single vector and the tail into (s0, e0)
template <bool PEN, bool STASH>
__global__ __launch_bounds__(256) void penalty_pass_kernel(float* g, const float* __restrict__ p, const float* __restrict__ om,
                                                       const float* __restrict__ an, int64_t n, float two_c, float* __restrict__ sg,
                                                       float* __restrict__ sp, float* __restrict__ sumsq, float* __restrict__ pen_out) {
  __shared__ float sm[4];
  float s0 = 0.f, s1 = 0.f, e0 = 0.f, e1 = 0.f;
  flat_pass2(n,
             [&](int64_t i, int64_t j) {
               const float4 a = penalty_pass4<PEN, STASH>(g, p, om, an, sg, sp, i, two_c, e0),
                            b = penalty_pass4<PEN, STASH>(g, p, om, an, sg, sp, j, two_c, e1);
               s0 += sq4(a);
               s1 += sq4(b);
             },
             [&](int64_t i) { s0 += sq4(penalty_pass4<PEN, STASH>(g, p, om, an, sg, sp, i, two_c, e0)); },
             [&](int64_t t) {
               float a = g[t];
               const float b = p[t];
               if (STASH) {
                 sg[t] = a;
                 sp[t] = b;
               }
               if (PEN) {
                 a = penalty1(a, b, om[t], an[t], two_c, e0);
                 g[t] = a;
               }
               s0 += a * a;
             });
  const float s = block_sum<256>(s0 + s1, sm);
  const float e = block_sum<256>(e0 + e1, sm);
  if (threadIdx.x == 0) {
    sumsq[blockIdx.x] = s;
    pen_out[blockIdx.x] = e;
  }
}

}  // namespace mafed
