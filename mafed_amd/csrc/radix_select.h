// What the per-segment radix selects share (PackNet's prune: packnet.hip; the TIES trim of the task-vector merge: merge.hip): the walk of
// one segment of a flat buffer, the 31-bit magnitude pattern and its 11 | 10 | 10 digits.  The scan that turns a histogram into the next
// prefix is mafed_packnet_scan for both.
#pragma once
#include "flat_pass.h"

namespace mafed {

constexpr int SELECT_BINS = 2048;   // bins of the first digit (11 bits), and the stride of a segment's histogram; the other two use 1024

__device__ __forceinline__ uint32_t mag_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// digit PASS of a pattern and the bits above it: 11 | 10 | 10
template <int PASS>
__device__ __forceinline__ uint32_t digit(uint32_t bits) { return PASS == 0 ? bits >> 20 : PASS == 1 ? (bits >> 10) & 1023u : bits & 1023u; }
template <int PASS>
__device__ __forceinline__ uint32_t above(uint32_t bits) { return PASS == 0 ? 0u : PASS == 1 ? bits >> 20 : bits >> 10; }

// This block's share of segment blockIdx.y = {offset, length} of a flat buffer of n elements, clipped to [0, n).  The segment may begin
// and end anywhere: whole(b) for the buffer's aligned fp32 vectors (elements b .. b + 3) that lie wholly inside it, one(i) for the
// elements of the two vectors that straddle an end.  Every element of a vector goes to the same thread, every element to exactly one.
template <class Whole, class One>
__device__ __forceinline__ void segment_walk(int64_t n, const int64_t* __restrict__ segments, Whole whole, One one) {
  int64_t lo = segments[2 * blockIdx.y], hi = lo + segments[2 * blockIdx.y + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n ? n : hi;
  if (hi <= lo) return;
  const int64_t v_hi = (hi + 3) / 4, stride = (int64_t)gridDim.x * flat_block_dim();
  for (int64_t v = lo / 4 + (int64_t)blockIdx.x * flat_block_dim() + threadIdx.x; v < v_hi; v += stride) {
    const int64_t base = v * 4;
    if (base >= lo && base + 4 <= hi) {
      whole(base);
    } else {
      for (int e = 0; e < 4; ++e) {
        const int64_t i = base + e;
        if (i >= lo && i < hi) one(i);
      }
    }
  }
}

static inline bool select_grid_ok(int n_segments, int blocks_per_segment) {
  return n_segments >= 0 && n_segments <= 65535 && blocks_per_segment >= 1 && blocks_per_segment <= 65535;
}

}  // namespace mafed
