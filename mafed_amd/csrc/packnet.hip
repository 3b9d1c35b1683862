// PackNet (Mallya & Lazebnik 2018) on the flat buffers.  State laid out like the parameters: the byte-wide owner
// map (owner[i] = the task that trained element i) and the fp32 anchor.  Element i is trainable in task t iff owner[i] == t.
//   mask_grad  (in front of the clip)     g = owner == t ? g : +0.0 in place; leaves the sum-of-squares partials of the g it leaves
//                                         (mafed_gradnorm_finish)                                          5 B read + 4 B written
//   hold       (behind the optimiser)     where owner != t:  p = anchor, shadow = bf16(anchor)             5 B read + at most 6 B written
//   view       (task_view)                where owner > k:   p = +0.0, shadow = 0                          1 B read + at most 6 B written
//   prune      (once per task)            per segment: tau = the k-th smallest |p| among owner == t, k = floor(f m); where owner == t and
//                                         |p| <= tau:  p = anchor = +0.0, shadow = 0, owner = t + 1
// The mask pass gives a thread 16 consecutive elements: one 16-byte owner load beside four 16-byte fp32 vectors.  The prune is
// a three-pass radix select (11 + 10 + 10 bits) on the 31-bit pattern of |p|: integer counts only, so the same bits on every run, and
// every scalar (m, k, tau, the number pruned) stays on the device.
#include "radix_select.h"

namespace mafed {

// ---- the per-step passes -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float keep1(float v, uint32_t own, uint32_t task) { return own == task ? v : 0.f; }

// one fp32 vector under its owner word (byte e = element e)
__device__ __forceinline__ float4 keep4(float4 a, uint32_t w, uint32_t task) {
  return make_float4(keep1(a.x, w & 0xffu, task), keep1(a.y, (w >> 8) & 0xffu, task), keep1(a.z, (w >> 16) & 0xffu, task), keep1(a.w, w >> 24, task));
}

// float4 unit u (elements 4u .. 4u + 3): all reads in front of the write; -> the masked vector
__device__ __forceinline__ float4 mask_unit(float* g, const uint8_t* owner, int64_t u, uint32_t task) {
  const uint32_t w = *reinterpret_cast<const uint32_t*>(owner + u * 4);
  const float4 a = keep4(load4(g + u * 4), w, task);
  store4(g + u * 4, a);
  return a;
}

// group q = 16 consecutive elements: one 16-byte owner load, four fp32 vectors; -> its sum of squares
__device__ __forceinline__ float mask_group(float* g, const uint8_t* owner, int64_t q, uint32_t task) {
  const uint4 o = *reinterpret_cast<const uint4*>(owner + q * 16);
  float* gq = g + q * 16;
  float4 a = load4(gq), b = load4(gq + 4), c = load4(gq + 8), d = load4(gq + 12);
  a = keep4(a, o.x, task);
  b = keep4(b, o.y, task);
  c = keep4(c, o.z, task);
  d = keep4(d, o.w, task);
  store4(gq, a);
  store4(gq + 4, b);
  store4(gq + 8, c);
  store4(gq + 12, d);
  return (sq4(a) + sq4(b)) + (sq4(c) + sq4(d));
}

// The loop of flat_pass.h one level up: its "elements" are the n / 4 fp32 vectors, so its vectors are the groups of 16 elements and its
// tail the up to three whole vectors behind the last group; the n % 4 elements behind those go to threads of block 0.
__global__ __launch_bounds__(256) void packnet_mask_kernel(float* g, const uint8_t* __restrict__ owner, int64_t n, uint32_t task,
                                                           float* __restrict__ sumsq) {
  __shared__ float sm[4];
  float s0 = 0.f, s1 = 0.f;
  const int64_t n4 = n / 4;
  flat_pass2(n4,
             [&](int64_t i, int64_t j) {
               const float a = mask_group(g, owner, i, task), b = mask_group(g, owner, j, task);
               s0 += a;
               s1 += b;
             },
             [&](int64_t i) { s0 += mask_group(g, owner, i, task); },
             [&](int64_t u) { s0 += sq4(mask_unit(g, owner, u, task)); });
  if (blockIdx.x == 0 && threadIdx.x < (n - n4 * 4)) {
    const int64_t t = n4 * 4 + threadIdx.x;
    const float a = keep1(g[t], owner[t], task);
    g[t] = a;
    s0 += a * a;
  }
  const float s = block_sum<256>(s0 + s1, sm);
  if (threadIdx.x == 0) sumsq[blockIdx.x] = s;
}

// hold: an element is held where owner != arg, and takes its anchor; view: held where owner > arg, and takes +0.0 (anchor is not read)
template <bool VIEW>
__device__ __forceinline__ bool held1(uint32_t own, uint32_t arg) { return VIEW ? own > arg : own != arg; }

template <bool VIEW>
__device__ __forceinline__ uint32_t held4(uint32_t w, uint32_t arg) {
  return (uint32_t)held1<VIEW>(w & 0xffu, arg) | ((uint32_t)held1<VIEW>((w >> 8) & 0xffu, arg) << 1) |
         ((uint32_t)held1<VIEW>((w >> 16) & 0xffu, arg) << 2) | ((uint32_t)held1<VIEW>(w >> 24, arg) << 3);
}

__device__ __forceinline__ void put1(float* p, bf16_t* shadow, int64_t i, float v) {
  p[i] = v;
  if (shadow) shadow[i] = f32_to_bf16(v);
}

// the stores of one fp32 vector: whole where every element is held, element by element where some are, none where none is
__device__ __forceinline__ void put_unit(float* p, bf16_t* shadow, int64_t u, uint32_t held, float4 a) {
  if (held == 15u) {
    store4(p + u * 4, a);
    if (shadow) store4(shadow + u * 4, a);
  } else if (held) {
    if (held & 1u) put1(p, shadow, u * 4, a.x);
    if (held & 2u) put1(p, shadow, u * 4 + 1, a.y);
    if (held & 4u) put1(p, shadow, u * 4 + 2, a.z);
    if (held & 8u) put1(p, shadow, u * 4 + 3, a.w);
  }
}

template <bool VIEW>
__device__ __forceinline__ void hold_unit(float* p, bf16_t* shadow, const uint8_t* owner, const float* anchor, int64_t u, uint32_t arg) {
  const uint32_t h = held4<VIEW>(*reinterpret_cast<const uint32_t*>(owner + u * 4), arg);
  if (!h) return;
  put_unit(p, shadow, u, h, VIEW ? make_float4(0.f, 0.f, 0.f, 0.f) : load4(anchor + u * 4));
}

// One fp32 vector per thread, not a group of 16: measured, the wide form is the slower one here -- its element
// stores of a vector with some held elements lie 64 bytes apart from lane to lane, these 16.  A vector without a held element reads its
// owner word and nothing else; p and the shadow are never read, so a trainable element cannot change.
template <bool VIEW>
__global__ __launch_bounds__(256) void packnet_hold_kernel(float* __restrict__ p, bf16_t* __restrict__ shadow, const uint8_t* __restrict__ owner,
                                                           const float* __restrict__ anchor, int64_t n, uint32_t arg) {
  flat_pass1(n, [&](int64_t u) { hold_unit<VIEW>(p, shadow, owner, anchor, u, arg); },
             [&](int64_t t) {
               if (held1<VIEW>(owner[t], arg)) put1(p, shadow, t, VIEW ? 0.f : anchor[t]);
             });
}

// ---- the prune: radix select per segment ---------------------------------------------------------------------------------------------
// This block's share of segment blockIdx.y (the walk, the pattern and its digits: radix_select.h): f(i, pattern of |p[i]|, owner[i]) for each of
// its elements inside [0, n).  The aligned fp32 vectors that lie wholly inside the segment are read as vectors (with their owner word),
// the two that straddle an end element by element.
template <class F>
__device__ __forceinline__ void segment_pass(const float* p, const uint8_t* owner, int64_t n, const int64_t* __restrict__ segments, F f) {
  segment_walk(n, segments,
               [&](int64_t base) {
                 const float4 a = load4(p + base);
                 const uint32_t w = *reinterpret_cast<const uint32_t*>(owner + base);
                 f(base, mag_bits(a.x), w & 0xffu);
                 f(base + 1, mag_bits(a.y), (w >> 8) & 0xffu);
                 f(base + 2, mag_bits(a.z), (w >> 16) & 0xffu);
                 f(base + 3, mag_bits(a.w), w >> 24);
               },
               [&](int64_t i) { f(i, mag_bits(p[i]), (uint32_t)owner[i]); });
}

template <int PASS>
__global__ __launch_bounds__(256) void packnet_hist_kernel(const float* __restrict__ p, const uint8_t* __restrict__ owner, int64_t n,
                                                           const int64_t* __restrict__ segments, uint32_t task, const int64_t* __restrict__ state,
                                                           uint32_t* hist) {
  constexpr int NB = PASS == 0 ? SELECT_BINS : 1024;
  __shared__ uint32_t h[NB];
  const int64_t* st = state + 4 * blockIdx.y;
  if (PASS > 0 && st[2] == 0) return;   // k == 0 in this segment (the whole block leaves)
  const uint32_t prefix = PASS > 0 ? (uint32_t)st[0] : 0u;
  for (int b = threadIdx.x; b < NB; b += 256) h[b] = 0u;
  __syncthreads();
  segment_pass(p, owner, n, segments, [&](int64_t, uint32_t bits, uint32_t own) {
    if (own == task && above<PASS>(bits) == prefix) atomicAdd(&h[digit<PASS>(bits)], 1u);
  });
  __syncthreads();
  uint32_t* out = hist + (int64_t)blockIdx.y * SELECT_BINS;
  for (int b = threadIdx.x; b < NB; b += 256) {
    const uint32_t c = h[b];
    if (c) atomicAdd(&out[b], c);
  }
}

// One block per segment.  Thread t owns the bins [t * PER, (t + 1) * PER); an inclusive scan of the threads' sums finds the thread, a walk
// of its bins the bin that holds the rank.
template <int PASS>
__global__ __launch_bounds__(256) void packnet_scan_kernel(const uint32_t* __restrict__ hist, double fraction, int64_t* state, int64_t* stats) {
  constexpr int NB = PASS == 0 ? SELECT_BINS : 1024, PER = NB / 256, SHIFT = PASS == 0 ? 0 : 10;
  __shared__ unsigned long long sm[256];
  int64_t* st = state + 4 * blockIdx.x;
  int64_t* out = stats + 4 * blockIdx.x;
  const int64_t active = PASS == 0 ? 1 : st[2], old_prefix = PASS == 0 ? 0 : st[0];
  int64_t rank = PASS == 0 ? 0 : st[1];
  if (!active) return;
  const uint32_t* h = hist + (int64_t)blockIdx.x * SELECT_BINS + threadIdx.x * PER;
  uint32_t c[PER];
  unsigned long long mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = h[j];
    mine += c[j];
  }
  sm[threadIdx.x] = mine;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned long long v = (int)threadIdx.x >= d ? sm[threadIdx.x - d] : 0ull;
    __syncthreads();
    sm[threadIdx.x] += v;
    __syncthreads();
  }
  const int64_t incl = (int64_t)sm[threadIdx.x], excl = incl - (int64_t)mine;
  if (PASS == 0) {
    const int64_t m = (int64_t)sm[255];
    rank = (int64_t)floor(fraction * (double)m);
    rank = rank > m ? m : rank < 0 ? 0 : rank;
    if (threadIdx.x == 0) {
      out[0] = m;
      out[1] = rank;
      out[2] = 0;
      out[3] = 0;
      st[0] = 0;
      st[1] = 0;
      st[2] = rank > 0;
      st[3] = 0;
    }
    // (thread 0 writes st[0], st[1] before the barrier below; the thread that finds the bin writes them behind it)
  }
  __syncthreads();
  if (rank > 0 && excl < rank && rank <= incl) {
    int64_t cum = excl;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (rank > cum && rank <= cum + (int64_t)c[j]) {
        const int64_t prefix = (old_prefix << SHIFT) | (int64_t)(threadIdx.x * PER + j);
        st[0] = prefix;
        st[1] = rank - cum;
        if (PASS == 2) out[3] = prefix;
      }
      cum += (int64_t)c[j];
    }
  }
}

__global__ __launch_bounds__(256) void packnet_apply_kernel(float* p, bf16_t* shadow, uint8_t* owner, float* anchor, int64_t n,
                                                            const int64_t* __restrict__ segments, uint32_t task, const int64_t* __restrict__ state,
                                                            int64_t* stats) {
  __shared__ unsigned int total;
  const int64_t* st = state + 4 * blockIdx.y;
  if (st[2] == 0) return;
  const uint32_t tau = (uint32_t)st[0];
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  unsigned int mine = 0u;
  segment_pass(p, owner, n, segments, [&](int64_t i, uint32_t bits, uint32_t own) {
    if (own == task && bits <= tau) {
      p[i] = 0.f;
      anchor[i] = 0.f;
      owner[i] = (uint8_t)(task + 1u);
      if (shadow) shadow[i] = (bf16_t)0;
      ++mine;
    }
  });
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 4 * blockIdx.y + 2), (unsigned long long)total);
}

}  // namespace mafed

using namespace mafed;

extern "C" int mafed_packnet_blocks(int64_t n) { return flat_blocks(n, FLAT_BLOCKS_CAP); }

extern "C" int mafed_packnet_mask_grad(float* g, const uint8_t* owner, int64_t n, int task, float* sumsq_partials, void* stream) {
  MAFED_CHECK_ARG(sumsq_partials && n >= 0 && task >= 0 && task <= 255 && (n == 0 || (g && owner)), "packnet_mask_grad: bad arguments");
  MAFED_CHECK_ARG(aligned16({g, owner}), "packnet_mask_grad: buffers must be 16-byte aligned");
  const dim3 grid((unsigned)mafed_packnet_blocks(n));   // (n == 0: one block that writes a zero partial)
  launch(K_PACKNET, (double)n * 9.0, packnet_mask_kernel, grid, dim3(256), 0, as_stream(stream), g, owner, n, (uint32_t)task, sumsq_partials);
  MAFED_CHECK_LAUNCH("packnet_mask_grad");
  return MAFED_OK;
}

extern "C" int mafed_packnet_hold(float* p, void* shadow, const uint8_t* owner, const float* anchor, int64_t n, int task, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && task >= 0 && task <= 255 && (n == 0 || (p && owner && anchor)), "packnet_hold: bad arguments");
  MAFED_CHECK_ARG(aligned16({p, shadow, owner, anchor}), "packnet_hold: buffers must be 16-byte aligned");
  if (n == 0) return MAFED_OK;
  launch(K_PACKNET, (double)n * (shadow ? 11.0 : 9.0), packnet_hold_kernel<false>, dim3((unsigned)mafed_packnet_blocks(n)), dim3(256), 0,
         as_stream(stream), p, (bf16_t*)shadow, owner, anchor, n, (uint32_t)task);
  MAFED_CHECK_LAUNCH("packnet_hold");
  return MAFED_OK;
}

extern "C" int mafed_packnet_view(float* p, void* shadow, const uint8_t* owner, int64_t n, int k, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && k >= 0 && k <= 255 && (n == 0 || (p && owner)), "packnet_view: bad arguments");
  MAFED_CHECK_ARG(aligned16({p, shadow, owner}), "packnet_view: buffers must be 16-byte aligned");
  if (n == 0) return MAFED_OK;
  launch(K_PACKNET, (double)n * (shadow ? 7.0 : 5.0), packnet_hold_kernel<true>, dim3((unsigned)mafed_packnet_blocks(n)), dim3(256), 0,
         as_stream(stream), p, (bf16_t*)shadow, owner, (const float*)nullptr, n, (uint32_t)k);
  MAFED_CHECK_LAUNCH("packnet_view");
  return MAFED_OK;
}

extern "C" int mafed_packnet_hist(const float* p, const uint8_t* owner, int64_t n, const int64_t* segments, int n_segments, int blocks_per_segment,
                                  int task, int pass, const int64_t* state, uint32_t* hist, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && select_grid_ok(n_segments, blocks_per_segment) && task >= 0 && task <= 254 && pass >= 0 && pass <= 2,
                  "packnet_hist: bad arguments (0 <= task <= 254, pass 0 .. 2, at most 65535 segments and blocks per segment)");
  MAFED_CHECK_ARG(n_segments == 0 || (segments && state && hist && (n == 0 || (p && owner))), "packnet_hist: null pointer");
  MAFED_CHECK_ARG(aligned16({p, owner}), "packnet_hist: buffers must be 16-byte aligned");
  if (n_segments == 0) return MAFED_OK;
  if (hipMemsetAsync(hist, 0, (size_t)n_segments * SELECT_BINS * sizeof(uint32_t), as_stream(stream)) != hipSuccess) {
    set_error("packnet_hist: clearing the histograms failed");
    return MAFED_ELAUNCH;
  }
  const dim3 grid((unsigned)blocks_per_segment, (unsigned)n_segments);
  auto go = [&](auto kernel) { launch(K_PACKNET, 0.0, kernel, grid, dim3(256), 0, as_stream(stream), p, owner, n, segments, (uint32_t)task, state, hist); };
  if (pass == 0) go(packnet_hist_kernel<0>);
  else if (pass == 1) go(packnet_hist_kernel<1>);
  else go(packnet_hist_kernel<2>);
  MAFED_CHECK_LAUNCH("packnet_hist");
  return MAFED_OK;
}

extern "C" int mafed_packnet_scan(const uint32_t* hist, int n_segments, int pass, double fraction, int64_t* state, int64_t* stats, void* stream) {
  MAFED_CHECK_ARG(n_segments >= 0 && pass >= 0 && pass <= 2 && fraction >= 0.0 && fraction <= 1.0,
                  "packnet_scan: bad arguments (pass 0 .. 2, fraction in [0, 1])");
  MAFED_CHECK_ARG(n_segments == 0 || (hist && state && stats), "packnet_scan: null pointer");
  if (n_segments == 0) return MAFED_OK;
  auto go = [&](auto kernel) { launch(K_PACKNET, 0.0, kernel, dim3((unsigned)n_segments), dim3(256), 0, as_stream(stream), hist, fraction, state, stats); };
  if (pass == 0) go(packnet_scan_kernel<0>);
  else if (pass == 1) go(packnet_scan_kernel<1>);
  else go(packnet_scan_kernel<2>);
  MAFED_CHECK_LAUNCH("packnet_scan");
  return MAFED_OK;
}

extern "C" int mafed_packnet_apply(float* p, void* shadow, uint8_t* owner, float* anchor, int64_t n, const int64_t* segments, int n_segments,
                                   int blocks_per_segment, int task, const int64_t* state, int64_t* stats, void* stream) {
  MAFED_CHECK_ARG(n >= 0 && select_grid_ok(n_segments, blocks_per_segment) && task >= 0 && task <= 254,
                  "packnet_apply: bad arguments (0 <= task <= 254, at most 65535 segments and blocks per segment)");
  MAFED_CHECK_ARG(n_segments == 0 || (segments && state && stats && (n == 0 || (p && owner && anchor))), "packnet_apply: null pointer");
  MAFED_CHECK_ARG(aligned16({p, shadow, owner, anchor}), "packnet_apply: buffers must be 16-byte aligned");
  if (n_segments == 0) return MAFED_OK;
  launch(K_PACKNET, 0.0, packnet_apply_kernel, dim3((unsigned)blocks_per_segment, (unsigned)n_segments), dim3(256), 0, as_stream(stream), p,
         (bf16_t*)shadow, owner, anchor, n, segments, (uint32_t)task, state, stats);
  MAFED_CHECK_LAUNCH("packnet_apply");
  return MAFED_OK;
}
