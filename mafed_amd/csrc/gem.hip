// GEM (Lopez-Paz & Ranzato, 2017) on the flat fp32 gradient buffer: the window's gradient g against the gradients
// r_1 .. r_K (K <= 8) of one memory batch per finished task,
//   gram[a][b] = sum x_a x_b  (x_0 = g, x_k = r_k; kept in fp64)     q_k = gram[0][k]     P = gram[1..K][1..K] + eps I
//   every q_k >= 0: v = 0, g stays as it is.   Else v = argmin 1/2 v'Pv + q'v s.t. v_k >= margin and g~ = g + sum_k v_k r_k.
// Two HBM-bound passes, (K + 1) 4 and (K + 2) 4 bytes per parameter (8 when nothing is violated), and between them a one-block exact
// solve: one candidate support per thread.  Every scalar stays on the device (gram64, stats12) and the second pass leaves the
// sum-of-squares partials of g~ for the clip norm (mafed_gradnorm_finish), which then does not read the buffer again.
#include <math.h>

#include "flat_pass.h"

namespace mafed {

constexpr int GEM_MAX_REFS = 8;

// the K reference buffers, by value in the kernel arguments: there is no device pointer table to keep alive
struct GemRefs {
  const float* p[GEM_MAX_REFS];
};

// index of the pair (a, b), a <= b, among the NV (NV + 1) / 2 pairs of NV vectors, row by row
__host__ __device__ constexpr int gem_pair(int a, int b, int nv) { return a * nv - a * (a - 1) / 2 + (b - a); }
__host__ __device__ constexpr int gem_pairs(int K) { return (K + 1) * (K + 2) / 2; }

template <int K>
__device__ __forceinline__ void gram_load(const float* g, const GemRefs& refs, int64_t i4, float4 (&x)[K + 1]) {
  x[0] = load4(g + i4 * 4);
#pragma unroll
  for (int k = 0; k < K; ++k) x[k + 1] = load4(refs.p[k] + i4 * 4);
}

template <int K>
__device__ __forceinline__ void gram_add(const float4 (&x)[K + 1], float (&acc)[gem_pairs(K)]) {
#pragma unroll
  for (int a = 0; a <= K; ++a) {
#pragma unroll
    for (int b = a; b <= K; ++b) acc[gem_pair(a, b, K + 1)] += dot4(x[a], x[b]);
  }
}

// partial[p * gridDim.x + blk] = this block's share of the pair p's sum.  One accumulator per pair and thread, in registers (the
// kernel is instantiated per K); up to K = 3 a trip loads two vectors of every buffer in front of its sums (as many loads in flight
// as agem_dots has), beyond that the K + 1 >= 5 buffers are the loads in flight.
template <int K>
__global__ __launch_bounds__(256) void gem_gram_partial_kernel(const float* __restrict__ g, const GemRefs refs, int64_t n,
                                                               float* __restrict__ partial) {
  constexpr int NP = gem_pairs(K);
  __shared__ float sm[4];
  float acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.f;
  auto one = [&](int64_t i) {
    float4 x[K + 1];
    gram_load<K>(g, refs, i, x);
    gram_add<K>(x, acc);
  };
  auto tail = [&](int64_t t) {
    float x[K + 1];
    x[0] = g[t];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k + 1] = refs.p[k][t];
#pragma unroll
    for (int a = 0; a <= K; ++a) {
#pragma unroll
      for (int b = a; b <= K; ++b) acc[gem_pair(a, b, K + 1)] += x[a] * x[b];
    }
  };
  if constexpr (K <= 3) {
    flat_pass2(n,
               [&](int64_t i, int64_t j) {
                 float4 x[K + 1], y[K + 1];
                 gram_load<K>(g, refs, i, x);
                 gram_load<K>(g, refs, j, y);
                 gram_add<K>(x, acc);
                 gram_add<K>(y, acc);
               },
               one, tail);
  } else {
    flat_pass1(n, one, tail);
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const float s = block_sum<256>(acc[p], sm);
    if (threadIdx.x == 0) partial[(int64_t)p * gridDim.x + blockIdx.x] = s;
  }
}

// One block: every pair's partials folded in double (index order per thread, then a fixed tree) -> the full symmetric matrix in fp64
__global__ __launch_bounds__(256) void gem_gram_finish_kernel(const float* __restrict__ partial, int nblk, int K, double* __restrict__ gram64) {
  __shared__ double sm[256];
  const int nv = K + 1;
  for (int a = 0; a < nv; ++a) {
    for (int b = a; b < nv; ++b) {
      double mine[1];
      fold_partials_f64(partial + (int64_t)gem_pair(a, b, nv) * nblk, nblk, mine);
      const double s = block_sum_f64(mine[0], sm);
      if (threadIdx.x == 0) {
        gram64[a * nv + b] = s;
        gram64[b * nv + a] = s;
      }
    }
  }
}

// The exact solve (one block, fp64): thread t < 2^K takes the support S = t read as a bit mask.  The K x K system is embedded in a
// fixed 8 x 8 one whose rows outside S are the identity's with a zero right-hand side -- the same numbers on S, u = 0 off it, and
// every loop has constant bounds, so L and u stay in registers.
//   u = v - margin >= 0, q' = q + margin P 1;  P_SS u_S = -q'_S by Cholesky; S is skipped if a pivot is <= 1e-12 max diag(P);
//   w = P u + q';  feasible iff min u_S >= -1e-9 max|u_S| and min w outside S >= -1e-9 max|q'|;
//   lowest objective 1/2 u'Pu + q''u among the feasible S, the lowest mask on a tie (thread 0 scans the masks in order).
__global__ __launch_bounds__(256) void gem_solve_kernel(const double* __restrict__ gram64, int K, float margin, float eps,
                                                        float* __restrict__ stats12) {
  constexpr int M = GEM_MAX_REFS;
  __shared__ double sP[M][M], sq[M], sqp[M], sobj[256], su[256][M];
  __shared__ int sflag[2];   // {a non-finite entry, a violated constraint}
  const int t = threadIdx.x, nv = K + 1;
  if (t < 2) sflag[t] = 0;
  __syncthreads();
  if (t < nv * nv && !isfinite(gram64[t])) sflag[0] = 1;
  if (t < M * M) {
    const int i = t / M, j = t % M;
    sP[i][j] = (i < K && j < K) ? gram64[(i + 1) * nv + (j + 1)] + (i == j ? (double)eps : 0.0) : (i == j ? 1.0 : 0.0);
  }
  if (t < M) {
    sq[t] = t < K ? gram64[t + 1] : 0.0;
    if (t < K && sq[t] < 0.0) sflag[1] = 1;
  }
  __syncthreads();
  if (t < M) {
    double s = 0.0;
    for (int j = 0; j < K; ++j) s += sP[t][j];
    sqp[t] = t < K ? sq[t] + (double)margin * s : 0.0;
  }
  __syncthreads();
  const bool bad = sflag[0] != 0, violated = bad || sflag[1] != 0;
  if (!violated || bad) {
    if (t < 12) stats12[t] = t < K && bad ? __builtin_nanf("") : (t == 8 && bad ? 1.f : 0.f);
    return;
  }
  double maxdiag = 0.0, maxq = 0.0;
#pragma unroll
  for (int k = 0; k < M; ++k) {
    if (k < K) {
      maxdiag = fmax(maxdiag, sP[k][k]);
      maxq = fmax(maxq, fabs(sqp[k]));
    }
  }
  double obj = INFINITY;   // infeasible, skipped or no subset of 1 .. K
  double u[M];
#pragma unroll
  for (int k = 0; k < M; ++k) u[k] = 0.0;
  if (t < (1 << K)) {
    const unsigned S = (unsigned)t;
    bool ok = true;
    double L[M][M];   // lower triangle, constant indices throughout
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const bool in_j = (S >> j) & 1u;
      double d = in_j ? sP[j][j] : 1.0;
#pragma unroll
      for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
      if (in_j && !(d > 1e-12 * maxdiag)) ok = false;
      const double ljj = sqrt(d);
      L[j][j] = ljj;
#pragma unroll
      for (int i = j + 1; i < M; ++i) {
        double s = (in_j && ((S >> i) & 1u)) ? sP[i][j] : 0.0;
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
        L[i][j] = s / ljj;
      }
    }
    // L y = -q'_S, L' u = y
    double y[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double s = ((S >> i) & 1u) ? -sqp[i] : 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < M; ++k) s -= L[k][i] * u[k];
      u[i] = ((S >> i) & 1u) ? s / L[i][i] : 0.0;
    }
    double minu = INFINITY, maxu = 0.0, minw = INFINITY, o = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if (i < K) {
        double w = sqp[i];
#pragma unroll
        for (int j = 0; j < M; ++j) w += sP[i][j] * u[j];
        if ((S >> i) & 1u) {
          minu = fmin(minu, u[i]);
          maxu = fmax(maxu, fabs(u[i]));
        } else {
          minw = fmin(minw, w);
        }
        o += u[i] * (0.5 * (w - sqp[i]) + sqp[i]);
      }
    }
    // (a NaN anywhere fails one of the comparisons: fmin / fmax drop it, the objective does not)
    ok = ok && minu >= -1e-9 * maxu && minw >= -1e-9 * maxq && isfinite(o);
    if (ok) obj = o;
  }
  sobj[t] = obj;
#pragma unroll
  for (int k = 0; k < M; ++k) su[t][k] = u[k];
  __syncthreads();
  if (t == 0) {
    int best = -1;
    double bo = INFINITY;
    for (int s = 0; s < (1 << K); ++s) {
      if (sobj[s] < bo) {
        bo = sobj[s];
        best = s;
      }
    }
    for (int k = 0; k < M; ++k) {
      float v = 0.f;
      if (k < K) v = best < 0 ? __builtin_nanf("") : (float)(fmax(su[best][k], 0.0) + (double)margin);
      stats12[k] = v;
    }
    stats12[8] = 1.f;
    stats12[9] = best < 0 ? 0.f : (float)__popc((unsigned)best);
    stats12[10] = 0.f;
    stats12[11] = 0.f;
  }
}

// One vector of g~ = g + sum_k v_k r_k: acc = g, then for k ascending acc = fma(v_k, r_k, acc).  KEEP selects g itself and reads no
// ref: g + 0 r would turn -0.0 into +0.0 and an infinite r into NaN.
template <int K, bool KEEP>
__device__ __forceinline__ float4 gem_project4(const float* g, const GemRefs& refs, int64_t i4, const float (&v)[K]) {
  float4 a = load4(g + i4 * 4);
  if (KEEP) return a;
  float4 r[K];
#pragma unroll
  for (int k = 0; k < K; ++k) r[k] = load4(refs.p[k] + i4 * 4);
#pragma unroll
  for (int k = 0; k < K; ++k) a = make_float4(fmaf(v[k], r[k].x, a.x), fmaf(v[k], r[k].y, a.y), fmaf(v[k], r[k].z, a.z), fmaf(v[k], r[k].w, a.w));
  return a;
}

// This thread's share of out = g~ -> its share of sum out^2.  out may alias g or any ref: every element is read and written by the
// same thread, all reads of a trip in front of its writes -- hence no __restrict__ on g, the refs and out.
template <int K, bool KEEP>
__device__ __forceinline__ float gem_project_pass(const float* g, const GemRefs& refs, float* out, int64_t n, const float (&v)[K]) {
  float s0 = 0.f, s1 = 0.f;
  flat_pass2(n,
             [&](int64_t i, int64_t j) {
               const float4 a = gem_project4<K, KEEP>(g, refs, i, v), b = gem_project4<K, KEEP>(g, refs, j, v);
               store4(out + i * 4, a);
               store4(out + j * 4, b);
               s0 += sq4(a);
               s1 += sq4(b);
             },
             [&](int64_t i) {
               const float4 a = gem_project4<K, KEEP>(g, refs, i, v);
               store4(out + i * 4, a);
               s0 += sq4(a);
             },
             [&](int64_t t) {
               float a = g[t];
               if (!KEEP) {
                 float r[K];
#pragma unroll
                 for (int k = 0; k < K; ++k) r[k] = refs.p[k][t];
#pragma unroll
                 for (int k = 0; k < K; ++k) a = fmaf(v[k], r[k], a);
               }
               out[t] = a;
               s0 += a * a;
             });
  return s0 + s1;
}

// out = g + sum_k stats12[k] refs[k] where stats12[8] != 0, else out = g; sumsq[b] = this block's share of sum out^2 (or null)
template <int K>
__global__ __launch_bounds__(256) void gem_project_kernel(const float* g, const GemRefs refs, float* out, int64_t n,
                                                          const float* __restrict__ stats12, float* __restrict__ sumsq) {
  __shared__ float sm[4];
  float v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = stats12[k];
  // (uniform over the grid)
  const float mine = stats12[8] == 0.f ? gem_project_pass<K, true>(g, refs, out, n, v) : gem_project_pass<K, false>(g, refs, out, n, v);
  if (sumsq) {
    const float s = block_sum<256>(mine, sm);
    if (threadIdx.x == 0) sumsq[blockIdx.x] = s;
  }
}

template <int K>
static void launch_gram(const float* g, const GemRefs& refs, int64_t n, float* partial, int nb, hipStream_t st) {
  launch(K_GRADNORM, (double)n * 4.0 * (K + 1), gem_gram_partial_kernel<K>, dim3((unsigned)nb), dim3(256), 0, st, g, refs, n, partial);
}

template <int K>
static void launch_project(const float* g, const GemRefs& refs, float* out, int64_t n, const float* stats12, float* sumsq, int nb,
                           hipStream_t st) {
  launch(K_GRADNORM, (double)n * 4.0 * (K + 2), gem_project_kernel<K>, dim3((unsigned)nb), dim3(256), 0, st, g, refs, out, n, stats12, sumsq);
}

// refs (a host array of K device pointers) -> the by-value argument; false on a null or misaligned ref among the first K
static bool gem_refs(const float* const* refs, int K, bool need, GemRefs* out) {
  for (int k = 0; k < GEM_MAX_REFS; ++k) out->p[k] = k < K ? refs[k] : nullptr;
  for (int k = 0; k < K; ++k) {
    if (need && !refs[k]) return false;
  }
  return true;
}

}  // namespace mafed

using namespace mafed;

#define GEM_DISPATCH_K(K, CALL)   \
  switch (K) {                    \
    case 1: CALL(1); break;       \
    case 2: CALL(2); break;       \
    case 3: CALL(3); break;       \
    case 4: CALL(4); break;       \
    case 5: CALL(5); break;       \
    case 6: CALL(6); break;       \
    case 7: CALL(7); break;       \
    default: CALL(8); break;      \
  }

extern "C" int mafed_gem_blocks(int64_t n) { return flat_blocks(n, FLAT_BLOCKS_CAP); }

extern "C" size_t mafed_gem_workspace_bytes(int64_t n, int K) {
  (void)n;
  if (K < 1 || K > GEM_MAX_REFS) return 0;
  return (size_t)gem_pairs(K) * FLAT_BLOCKS_CAP * sizeof(float);
}

extern "C" int mafed_gem_gram(const float* g, const float* const* refs, int K, int64_t n, double* gram64, void* workspace,
                              size_t workspace_bytes, void* stream) {
  MAFED_CHECK_ARG(K >= 1 && K <= GEM_MAX_REFS, "gem_gram: K = %d outside 1 .. %d", K, GEM_MAX_REFS);
  MAFED_CHECK_ARG(gram64 && refs && n >= 0 && (n == 0 || g), "gem_gram: bad arguments");
  GemRefs r;
  MAFED_CHECK_ARG(gem_refs(refs, K, n > 0, &r), "gem_gram: a null reference buffer among the first %d", K);
  MAFED_CHECK_ARG(aligned16({g, r.p[0], r.p[1], r.p[2], r.p[3], r.p[4], r.p[5], r.p[6], r.p[7]}), "gem_gram: buffers must be 16-byte aligned");
  if (!workspace || workspace_bytes < mafed_gem_workspace_bytes(n, K)) {
    set_error("gem_gram: workspace %zu < %zu", workspace_bytes, mafed_gem_workspace_bytes(n, K));
    return MAFED_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int nb = mafed_gem_blocks(n);   // (n == 0: one block that writes zero partials)
  float* partial = (float*)workspace;
#define GEM_GRAM(KK) launch_gram<KK>(g, r, n, partial, nb, st)
  GEM_DISPATCH_K(K, GEM_GRAM)
#undef GEM_GRAM
  MAFED_CHECK_LAUNCH("gem_gram(partial)");
  launch(K_SMALL, 0.0, gem_gram_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, nb, K, gram64);
  MAFED_CHECK_LAUNCH("gem_gram(finish)");
  return MAFED_OK;
}

extern "C" int mafed_gem_solve(const double* gram64, int K, float margin, float eps, float* stats12, void* stream) {
  MAFED_CHECK_ARG(K >= 1 && K <= GEM_MAX_REFS, "gem_solve: K = %d outside 1 .. %d", K, GEM_MAX_REFS);
  MAFED_CHECK_ARG(gram64 && stats12, "gem_solve: bad arguments");
  MAFED_CHECK_ARG(margin >= 0.f && eps >= 0.f, "gem_solve: margin and eps must be >= 0");
  launch(K_SMALL, 0.0, gem_solve_kernel, dim3(1), dim3(256), 0, as_stream(stream), gram64, K, margin, eps, stats12);
  MAFED_CHECK_LAUNCH("gem_solve");
  return MAFED_OK;
}

extern "C" int mafed_gem_project(const float* g, const float* const* refs, int K, float* out, int64_t n, const float* stats12,
                                 float* sumsq_partials, void* stream) {
  MAFED_CHECK_ARG(K >= 1 && K <= GEM_MAX_REFS, "gem_project: K = %d outside 1 .. %d", K, GEM_MAX_REFS);
  MAFED_CHECK_ARG(stats12 && refs && n >= 0 && (n == 0 || (g && out)), "gem_project: bad arguments");
  GemRefs r;
  MAFED_CHECK_ARG(gem_refs(refs, K, n > 0, &r), "gem_project: a null reference buffer among the first %d", K);
  MAFED_CHECK_ARG(aligned16({g, out, r.p[0], r.p[1], r.p[2], r.p[3], r.p[4], r.p[5], r.p[6], r.p[7]}),
                  "gem_project: buffers must be 16-byte aligned");
  if (n == 0 && !sumsq_partials) return MAFED_OK;
  hipStream_t st = as_stream(stream);
  const int nb = mafed_gem_blocks(n);
#define GEM_PROJECT(KK) launch_project<KK>(g, r, out, n, stats12, sumsq_partials, nb, st)
  GEM_DISPATCH_K(K, GEM_PROJECT)
#undef GEM_PROJECT
  MAFED_CHECK_LAUNCH("gem_project");
  return MAFED_OK;
}
