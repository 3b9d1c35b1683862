// A-GEM (Chaudhry et al., 2019) on the flat fp32 gradient buffer: the window's gradient g is projected against
// the gradient r of one replay-memory batch,
//   dot = sum g_i r_i    rsq = sum r_i^2    alpha = dot / rsq if dot < 0 and rsq > 0, else 0    g'_i = g_i - alpha r_i
// Two HBM-bound passes, 8 and 12 bytes per parameter (8 and 8 when nothing is violated); every scalar stays on the device (stats4) and
// the second pass leaves the sum-of-squares partials of g' for the clip norm (mafed_gradnorm_finish), which then does not read the
// buffer again.
#include "flat_pass.h"

namespace mafed {

// partial[b] = this block's share of sum g r, partial[gridDim.x + b] = its share of sum r r.  The vectors of a pair go into (d0, q0)
// and (d1, q1), a single vector and the tail into (d0, q0).  The loop of flat_pass2 written out: through the callables hipcc packs the
// two sums into other lanes and contracts the other product of each a.x b.x + a.y b.y into the fma -- other bits in both sums.
__global__ __launch_bounds__(256) void agem_dots_partial_kernel(const float* __restrict__ g, const float* __restrict__ r, int64_t n,
                                                                float* __restrict__ partial) {
  __shared__ float sm[4];
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float d0 = 0.f, d1 = 0.f, q0 = 0.f, q1 = 0.f;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const float4 ga = load4(g + i * 4), ra = load4(r + i * 4), gb = load4(g + (i + stride) * 4), rb = load4(r + (i + stride) * 4);
    d0 += dot4(ga, ra); q0 += sq4(ra);
    d1 += dot4(gb, rb); q1 += sq4(rb);
  }
  for (; i < n4; i += stride) {
    const float4 ga = load4(g + i * 4), ra = load4(r + i * 4);
    d0 += dot4(ga, ra); q0 += sq4(ra);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n - n4 * 4)) {
    const int64_t j = n4 * 4 + threadIdx.x;
    d0 += g[j] * r[j];
    q0 += r[j] * r[j];
  }
  const float d = block_sum<256>(d0 + d1, sm);
  const float q = block_sum<256>(q0 + q1, sm);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = d;
    partial[gridDim.x + blockIdx.x] = q;
  }
}

// One block: the partials folded in double (index order per thread, then a fixed tree) -> stats4 = {dot, rsq, alpha, violated}.
// A non-finite dot or rsq is not hidden: alpha = NaN (and violated = 1: the projection pass then poisons g', whose norm trips the
// optimiser's non-finite guard).
__global__ __launch_bounds__(256) void agem_dots_finish_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ stats4) {
  __shared__ double sm[256];
  double mine[2];
  fold_partials_f64(partial, nblk, mine);
  const double d = block_sum_f64(mine[0], sm);
  const double q = block_sum_f64(mine[1], sm);
  if (threadIdx.x == 0) {
    const float dot = (float)d, rsq = (float)q;
    const bool finite = isfinite(dot) && isfinite(rsq);
    const bool violated = !finite || (dot < 0.f && rsq > 0.f);
    stats4[0] = dot;
    stats4[1] = rsq;
    stats4[2] = !finite ? __builtin_nanf("") : (violated ? dot / rsq : 0.f);
    stats4[3] = violated ? 1.f : 0.f;
  }
}

// One element of g' = g - alpha r.  KEEP (alpha == 0) selects g itself and does not read r: g - 0 * r would turn -0.0 into +0.0 and
// an infinite r into NaN, and the common step without a violation moves 8 bytes per parameter instead of 12.
template <bool KEEP>
__device__ __forceinline__ float4 project4(const float* g, const float* r, int64_t i4, float alpha) {
  const float4 a = load4(g + i4 * 4);
  if (KEEP) return a;
  const float4 b = load4(r + i4 * 4);
  return make_float4(fmaf(-alpha, b.x, a.x), fmaf(-alpha, b.y, a.y), fmaf(-alpha, b.z, a.z), fmaf(-alpha, b.w, a.w));
}

// This thread's share of out = g - alpha r -> its share of sum out^2 (the vectors of a pair into s0 and s1, a single vector and the tail
// into s0).  out may alias r (or g): every element is read and written by the same thread, all reads of a trip in front of its writes --
// hence no __restrict__ on g, r and out.
template <bool KEEP>
__device__ __forceinline__ float project_pass(const float* g, const float* r, float* out, int64_t n, float alpha) {
  float s0 = 0.f, s1 = 0.f;
  flat_pass2(n,
             [&](int64_t i, int64_t j) {
               const float4 a = project4<KEEP>(g, r, i, alpha), b = project4<KEEP>(g, r, j, alpha);
               store4(out + i * 4, a);
               store4(out + j * 4, b);
               s0 += sq4(a);
               s1 += sq4(b);
             },
             [&](int64_t i) {
               const float4 a = project4<KEEP>(g, r, i, alpha);
               store4(out + i * 4, a);
               s0 += sq4(a);
             },
             [&](int64_t t) {
               const float a = KEEP ? g[t] : fmaf(-alpha, r[t], g[t]);
               out[t] = a;
               s0 += a * a;
             });
  return s0 + s1;
}

// out = g - alpha r with alpha = stats4[2]; sumsq[b] = this block's share of sum out^2 (sumsq may be null)
__global__ __launch_bounds__(256) void agem_project_kernel(const float* g, const float* r, float* out, int64_t n,
                                                           const float* __restrict__ stats4, float* __restrict__ sumsq) {
  __shared__ float sm[4];
  const float alpha = stats4[2];
  // (uniform over the grid; NaN != 0: a poisoned alpha is applied, not kept back)
  const float mine = alpha == 0.f ? project_pass<true>(g, r, out, n, alpha) : project_pass<false>(g, r, out, n, alpha);
  if (sumsq) {
    const float s = block_sum<256>(mine, sm);
    if (threadIdx.x == 0) sumsq[blockIdx.x] = s;
  }
}

}  // namespace mafed

using namespace mafed;

extern "C" int mafed_agem_blocks(int64_t n) { return flat_blocks(n, FLAT_BLOCKS_CAP); }

extern "C" size_t mafed_agem_workspace_bytes(int64_t n) { (void)n; return (size_t)2 * FLAT_BLOCKS_CAP * sizeof(float); }

extern "C" int mafed_agem_dots(const float* g, const float* r, int64_t n, float* stats4, void* workspace, size_t workspace_bytes,
                               void* stream) {
  MAFED_CHECK_ARG(stats4 && n >= 0 && (n == 0 || (g && r)), "agem_dots: bad arguments");
  MAFED_CHECK_ARG(aligned16({g, r}), "agem_dots: buffers must be 16-byte aligned");
  if (!workspace || workspace_bytes < mafed_agem_workspace_bytes(n)) {
    set_error("agem_dots: workspace %zu < %zu", workspace_bytes, mafed_agem_workspace_bytes(n));
    return MAFED_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int nb = mafed_agem_blocks(n);   // (n == 0: one block that writes two zero partials)
  launch(K_GRADNORM, (double)n * 8.0, agem_dots_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, g, r, n, (float*)workspace);
  MAFED_CHECK_LAUNCH("agem_dots(partial)");
  launch(K_SMALL, 0.0, agem_dots_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, nb, stats4);
  MAFED_CHECK_LAUNCH("agem_dots(finish)");
  return MAFED_OK;
}

extern "C" int mafed_agem_project(const float* g, const float* r, float* out, int64_t n, const float* stats4, float* sumsq_partials,
                                  void* stream) {
  MAFED_CHECK_ARG(stats4 && n >= 0 && (n == 0 || (g && r && out)), "agem_project: bad arguments");
  MAFED_CHECK_ARG(aligned16({g, r, out}), "agem_project: buffers must be 16-byte aligned");
  if (n == 0 && !sumsq_partials) return MAFED_OK;
  launch(K_GRADNORM, (double)n * 12.0, agem_project_kernel, dim3((unsigned)mafed_agem_blocks(n)), dim3(256), 0, as_stream(stream), g, r, out, n,
         stats4, sumsq_partials);
  MAFED_CHECK_LAUNCH("agem_project");
  return MAFED_OK;
}
