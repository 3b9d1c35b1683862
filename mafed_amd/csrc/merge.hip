// Task-vector model merging on the flat buffers: task arithmetic (Ilharco et al. 2023), MagMax (Marczak et al. 2024)
// and TIES (Yadav et al. 2023), streaming -- the state is laid out like the parameters and does not grow with the number of tasks.
// With tau = fl(theta - base), one IEEE subtraction per element:
//   fold       sum:     acc = fl(acc + tau)                 magmax:  acc = |tau| > |acc| ? tau : acc  (strict: a tie keeps the earlier task;
//                                                                    a NaN tau never wins, a NaN acc never leaves)         12 B read + 4 B written
//   ties_hist  per segment: the histogram of digit `pass` of the 31-bit pattern of |tau| under the prefix in state (radix_select.h; the scan is
//              mafed_packnet_scan)                                                                                          8 B read
//   ties_fold  per segment: element i is kept iff r == 0 or pattern(|tau|) > tau_bits; on kept elements  tau > 0: pos += tau, npos += 1
//              tau < 0: neg += tau, nneg += 1;  stats[s][2] = the number kept                            18 B read + at most 10 B written
//   apply      d = acc, or for ties with s = fl(pos + neg):  s > 0: pos / npos   s < 0: neg / nneg   else +0.0;
//              p = fl(base + fl(scaling * d)), shadow = bf16(p)                                          8 or 14 B read + 4 or 6 B written
// Every product, sum and quotient is rounded on its own (contraction is off for this file: nothing becomes an FMA; __fdiv_rn), the
// counts are integers, so every pass gives the same bits on every run.  The two byte counters of element i are counts[2 i] (npos) and
// counts[2 i + 1] (nneg): a vector of four elements reads them with one 8-byte load.
#include "radix_select.h"

// hipcc contracts a * b + c into an FMA by default, and HIP's __fmul_rn / __fadd_rn do not stop it: they are plain operators compiled under the
// header's own contraction setting.  So the arithmetic below is written with plain operators and contraction is off for this file: every
// product and sum is an instruction of its own (the disassembly's only v_fma are the steps of the IEEE division in the TIES apply).
#pragma clang fp contract(off)

namespace mafed {

// ---- sum and magmax ------------------------------------------------------------------------------------------------------------------
template <bool MAGMAX>
__device__ __forceinline__ float fold1(float th, float b, float a) {
  const float t = (th - b);
  return MAGMAX ? (fabsf(t) > fabsf(a) ? t : a) : (a + t);
}

template <bool MAGMAX>
__device__ __forceinline__ float4 fold4(const float* theta, const float* base, const float* acc, int64_t u) {
  const float4 t = load4(theta + u * 4), b = load4(base + u * 4), a = load4(acc + u * 4);
  return make_float4(fold1<MAGMAX>(t.x, b.x, a.x), fold1<MAGMAX>(t.y, b.y, a.y), fold1<MAGMAX>(t.z, b.z, a.z), fold1<MAGMAX>(t.w, b.w, a.w));
}

template <bool MAGMAX>
__global__ __launch_bounds__(256) void merge_fold_kernel(const float* __restrict__ theta, const float* __restrict__ base, float* acc, int64_t n) {
  flat_pass2(n,
             [&](int64_t i, int64_t j) {
               const float4 a = fold4<MAGMAX>(theta, base, acc, i), b = fold4<MAGMAX>(theta, base, acc, j);
               store4(acc + i * 4, a);
               store4(acc + j * 4, b);
             },
             [&](int64_t i) { store4(acc + i * 4, fold4<MAGMAX>(theta, base, acc, i)); },
             [&](int64_t t) { acc[t] = fold1<MAGMAX>(theta[t], base[t], acc[t]); });
}

// ---- the TIES trim and fold ----------------------------------------------------------------------------------------------------------
// true where no vector of segment blockIdx.y falls to this block: the selection's grids are sized by the longest segment, and the model's
// tensors differ in length by four orders of magnitude
__device__ __forceinline__ bool segment_block_idle(int64_t n, const int64_t* __restrict__ segments) {
  int64_t lo = segments[2 * blockIdx.y], hi = lo + segments[2 * blockIdx.y + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n ? n : hi;
  return hi <= lo || lo / 4 + (int64_t)blockIdx.x * flat_block_dim() >= (hi + 3) / 4;
}

template <int PASS>
__global__ __launch_bounds__(256) void merge_ties_hist_kernel(const float* __restrict__ theta, const float* __restrict__ base, int64_t n,
                                                              const int64_t* __restrict__ segments, const int64_t* __restrict__ state, uint32_t* hist) {
  constexpr int NB = PASS == 0 ? SELECT_BINS : 1024;
  __shared__ uint32_t h[NB];
  const int64_t* st = state + 4 * blockIdx.y;
  if ((PASS > 0 && st[2] == 0) || segment_block_idle(n, segments)) return;   // r == 0 in this segment, or nothing to read (the whole block leaves)
  const uint32_t prefix = PASS > 0 ? (uint32_t)st[0] : 0u;
  for (int b = threadIdx.x; b < NB; b += 256) h[b] = 0u;
  __syncthreads();
  auto count = [&](float th, float b) {
    const uint32_t bits = mag_bits((th - b));
    if (above<PASS>(bits) == prefix) atomicAdd(&h[digit<PASS>(bits)], 1u);
  };
  segment_walk(n, segments,
               [&](int64_t e) {
                 const float4 t = load4(theta + e), b = load4(base + e);
                 count(t.x, b.x);
                 count(t.y, b.y);
                 count(t.z, b.z);
                 count(t.w, b.w);
               },
               [&](int64_t i) { count(theta[i], base[i]); });
  __syncthreads();
  uint32_t* out = hist + (int64_t)blockIdx.y * SELECT_BINS;
  for (int b = threadIdx.x; b < NB; b += 256) {
    const uint32_t c = h[b];
    if (c) atomicAdd(&out[b], c);
  }
}

// one element of the fold, in registers: the sums and the counter pair c = npos | nneg << 8 as the element leaves them
struct TiesElem {
  float pos, neg;
  uint32_t c;
  bool kept;
};

__device__ __forceinline__ TiesElem ties1(float th, float b, bool all, uint32_t tau_bits, float pos, float neg, uint32_t c) {
  const float t = (th - b);
  const bool kept = all || mag_bits(t) > tau_bits;
  const bool up = kept && t > 0.f, down = kept && t < 0.f;
  TiesElem r;
  r.pos = up ? (pos + t) : pos;
  r.neg = down ? (neg + t) : neg;
  r.c = up ? (c & 0xff00u) | ((c + 1u) & 0xffu) : down ? (c & 0x00ffu) | ((c + 0x100u) & 0xff00u) : c;
  r.kept = kept;
  return r;
}

__global__ __launch_bounds__(256) void merge_ties_fold_kernel(const float* __restrict__ theta, const float* __restrict__ base, float* pos, float* neg,
                                                              uint8_t* counts, int64_t n, const int64_t* __restrict__ segments,
                                                              const int64_t* __restrict__ state, int64_t* stats) {
  __shared__ unsigned int total;
  if (segment_block_idle(n, segments)) return;
  const int64_t* st = state + 4 * blockIdx.y;
  const bool all = st[2] == 0;   // r == 0: nothing is trimmed
  const uint32_t tau_bits = (uint32_t)st[0];
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  unsigned int mine = 0u;
  segment_walk(n, segments,
               [&](int64_t e) {
                 const float4 t = load4(theta + e), b = load4(base + e), p = load4(pos + e), q = load4(neg + e);
                 const uint2 c = *reinterpret_cast<const uint2*>(counts + 2 * e);
                 const TiesElem x = ties1(t.x, b.x, all, tau_bits, p.x, q.x, c.x & 0xffffu), y = ties1(t.y, b.y, all, tau_bits, p.y, q.y, c.x >> 16),
                                z = ties1(t.z, b.z, all, tau_bits, p.z, q.z, c.y & 0xffffu), w = ties1(t.w, b.w, all, tau_bits, p.w, q.w, c.y >> 16);
                 const unsigned int k = (unsigned)x.kept + (unsigned)y.kept + (unsigned)z.kept + (unsigned)w.kept;
                 mine += k;
                 if (k) {   // (a kept zero or NaN rewrites what stood there)
                   store4(pos + e, make_float4(x.pos, y.pos, z.pos, w.pos));
                   store4(neg + e, make_float4(x.neg, y.neg, z.neg, w.neg));
                   *reinterpret_cast<uint2*>(counts + 2 * e) = make_uint2(x.c | (y.c << 16), z.c | (w.c << 16));
                 }
               },
               [&](int64_t i) {
                 const TiesElem x = ties1(theta[i], base[i], all, tau_bits, pos[i], neg[i], (uint32_t)counts[2 * i] | ((uint32_t)counts[2 * i + 1] << 8));
                 if (x.kept) {
                   pos[i] = x.pos;
                   neg[i] = x.neg;
                   counts[2 * i] = (uint8_t)(x.c & 0xffu);
                   counts[2 * i + 1] = (uint8_t)(x.c >> 8);
                   ++mine;
                 }
               });
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 4 * blockIdx.y + 2), (unsigned long long)total);
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float apply1(float b, float d, float scaling) { return (b + (scaling * d)); }

// elect and mean: the sign of the summed mass decides, a dead heat (or a NaN) gives +0.0; c = npos | nneg << 8
__device__ __forceinline__ float ties_delta(float pos, float neg, uint32_t c) {
  const float s = (pos + neg);
  return s > 0.f ? __fdiv_rn(pos, (float)(c & 0xffu)) : s < 0.f ? __fdiv_rn(neg, (float)(c >> 8)) : 0.f;
}

template <bool TIES>
__device__ __forceinline__ float4 apply4(const float* base, const float* acc, const float* neg, const uint8_t* counts, int64_t u, float scaling) {
  const float4 b = load4(base + u * 4);
  float4 d = load4(acc + u * 4);
  if (TIES) {
    const float4 q = load4(neg + u * 4);
    const uint2 c = *reinterpret_cast<const uint2*>(counts + u * 8);
    d = make_float4(ties_delta(d.x, q.x, c.x & 0xffffu), ties_delta(d.y, q.y, c.x >> 16), ties_delta(d.z, q.z, c.y & 0xffffu),
                    ties_delta(d.w, q.w, c.y >> 16));
  }
  return make_float4(apply1(b.x, d.x, scaling), apply1(b.y, d.y, scaling), apply1(b.z, d.z, scaling), apply1(b.w, d.w, scaling));
}

__device__ __forceinline__ void put4(float* p, bf16_t* shadow, int64_t u, float4 v) {
  store4(p + u * 4, v);
  if (shadow) store4(shadow + u * 4, v);
}

// Two vectors in flight per thread, all reads of a trip in front of its writes (p carries no __restrict__: it may be one of the inputs)
template <bool TIES>
__global__ __launch_bounds__(256) void merge_apply_kernel(float* p, bf16_t* shadow, const float* base, const float* acc, const float* neg,
                                                          const uint8_t* counts, int64_t n, float scaling) {
  flat_pass2(n,
             [&](int64_t i, int64_t j) {
               const float4 a = apply4<TIES>(base, acc, neg, counts, i, scaling), b = apply4<TIES>(base, acc, neg, counts, j, scaling);
               put4(p, shadow, i, a);
               put4(p, shadow, j, b);
             },
             [&](int64_t i) { put4(p, shadow, i, apply4<TIES>(base, acc, neg, counts, i, scaling)); },
             [&](int64_t t) {
               const float d = TIES ? ties_delta(acc[t], neg[t], (uint32_t)counts[2 * t] | ((uint32_t)counts[2 * t + 1] << 8)) : acc[t];
               const float v = apply1(base[t], d, scaling);
               p[t] = v;
               if (shadow) shadow[t] = f32_to_bf16(v);
             });
}

}  // namespace mafed

using namespace mafed;

extern "C" int mafed_merge_fold(const float* theta, const float* base, float* acc, int64_t n, int rule, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && (rule == MAFED_MERGE_SUM || rule == MAFED_MERGE_MAGMAX) && (n == 0 || (theta && base && acc)),
                  "merge_fold: bad arguments (rule: sum or magmax)");
  MAFED_CHECK_ARG(aligned16({theta, base, acc}), "merge_fold: buffers must be 16-byte aligned");
  if (n == 0) return MAFED_OK;
  const dim3 grid((unsigned)flat_blocks(n, FLAT_BLOCKS_CAP));
  if (rule == MAFED_MERGE_MAGMAX) launch(K_MERGE, (double)n * 16.0, merge_fold_kernel<true>, grid, dim3(256), 0, as_stream(stream), theta, base, acc, n);
  else launch(K_MERGE, (double)n * 16.0, merge_fold_kernel<false>, grid, dim3(256), 0, as_stream(stream), theta, base, acc, n);
  MAFED_CHECK_LAUNCH("merge_fold");
  return MAFED_OK;
}

extern "C" int mafed_merge_ties_hist(const float* theta, const float* base, int64_t n, const int64_t* segments, int n_segments, int blocks_per_segment,
                                     int pass, const int64_t* state, uint32_t* hist, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && select_grid_ok(n_segments, blocks_per_segment) && pass >= 0 && pass <= 2,
                  "merge_ties_hist: bad arguments (pass 0 .. 2, at most 65535 segments and blocks per segment)");
  MAFED_CHECK_ARG(n_segments == 0 || (segments && state && hist && (n == 0 || (theta && base))), "merge_ties_hist: null pointer");
  MAFED_CHECK_ARG(aligned16({theta, base}), "merge_ties_hist: buffers must be 16-byte aligned");
  if (n_segments == 0) return MAFED_OK;
  if (hipMemsetAsync(hist, 0, (size_t)n_segments * SELECT_BINS * sizeof(uint32_t), as_stream(stream)) != hipSuccess) {
    set_error("merge_ties_hist: clearing the histograms failed");
    return MAFED_ELAUNCH;
  }
  const dim3 grid((unsigned)blocks_per_segment, (unsigned)n_segments);
  auto go = [&](auto kernel) { launch(K_MERGE, (double)n * 8.0, kernel, grid, dim3(256), 0, as_stream(stream), theta, base, n, segments, state, hist); };
  if (pass == 0) go(merge_ties_hist_kernel<0>);
  else if (pass == 1) go(merge_ties_hist_kernel<1>);
  else go(merge_ties_hist_kernel<2>);
  MAFED_CHECK_LAUNCH("merge_ties_hist");
  return MAFED_OK;
}

extern "C" int mafed_merge_ties_fold(const float* theta, const float* base, float* pos, float* neg, uint8_t* counts, int64_t n, const int64_t* segments,
                                     int n_segments, int blocks_per_segment, const int64_t* state, int64_t* stats, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && select_grid_ok(n_segments, blocks_per_segment),
                  "merge_ties_fold: bad arguments (at most 65535 segments and blocks per segment)");
  MAFED_CHECK_ARG(n_segments == 0 || (segments && state && stats && (n == 0 || (theta && base && pos && neg && counts))), "merge_ties_fold: null pointer");
  MAFED_CHECK_ARG(aligned16({theta, base, pos, neg, counts}), "merge_ties_fold: buffers must be 16-byte aligned");
  if (n_segments == 0) return MAFED_OK;
  launch(K_MERGE, (double)n * 28.0, merge_ties_fold_kernel, dim3((unsigned)blocks_per_segment, (unsigned)n_segments), dim3(256), 0, as_stream(stream), theta,
         base, pos, neg, counts, n, segments, state, stats);
  MAFED_CHECK_LAUNCH("merge_ties_fold");
  return MAFED_OK;
}

extern "C" int mafed_merge_apply(float* p, void* shadow, const float* base, const float* acc, const float* neg, const uint8_t* counts, int64_t n,
                                 int rule, float scaling, void* stream) {
  const bool ties = rule == MAFED_MERGE_TIES;
  MAFED_CHECK_ARG(n >= 0 && (ties || rule == MAFED_MERGE_SUM || rule == MAFED_MERGE_MAGMAX) && (n == 0 || (p && base && acc)),
                  "merge_apply: bad arguments (rule: sum, magmax or ties)");
  MAFED_CHECK_ARG(n == 0 || (ties == (neg != nullptr) && ties == (counts != nullptr)),
                  "merge_apply: neg and counts come with the ties rule, and only with it");
  MAFED_CHECK_ARG(aligned16({p, shadow, base, acc, neg, counts}), "merge_apply: buffers must be 16-byte aligned");
  if (n == 0) return MAFED_OK;
  const dim3 grid((unsigned)flat_blocks(n, FLAT_BLOCKS_CAP));
  const double bytes = (double)n * ((ties ? 18.0 : 12.0) + (shadow ? 2.0 : 0.0));
  if (ties)
    launch(K_MERGE, bytes, merge_apply_kernel<true>, grid, dim3(256), 0, as_stream(stream), p, (bf16_t*)shadow, base, acc, neg, counts, n, scaling);
  else
    launch(K_MERGE, bytes, merge_apply_kernel<false>, grid, dim3(256), 0, as_stream(stream), p, (bf16_t*)shadow, base, acc, neg, counts, n, scaling);
  MAFED_CHECK_LAUNCH("merge_apply");
  return MAFED_OK;
}
