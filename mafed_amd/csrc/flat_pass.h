// The one copy of what the HBM-bound passes over the flat fp32 buffers share (clip norm: optim.hip; EWC: ewc.hip; A-GEM: agem.hip; MAS: mas.hip;
// SI: si.hip): the grid-stride loops with their n % 4 tail, the grid size, the float4 dot, the double fold of a finish kernel and the
// entry points' alignment check.  A kernel's body shows its arithmetic and nothing else.
#pragma once
#include <initializer_list>

#include "common.h"

namespace mafed {

// Grid caps of the reducing passes (256 threads per block, 256 CUs).  2048 = 8 blocks per CU with two 16-byte vectors per stream in
// flight per thread; the clip norm's 1024 is older and nobody has measured whether the two need to differ.  Neither can change without
// changing results: the cap fixes the number of partials of a buffer and with it the order of the sum.
constexpr int NORM_BLOCKS_CAP = 1024, FLAT_BLOCKS_CAP = 2048;

// blocks of a pass over n elements: one per 1024 vectors (four 16-byte vectors per thread), at least 1, at most cap
static inline int flat_blocks(int64_t n, int cap) {
  const int64_t nb = cdiv(n / 4 + 1, 256 * 4);
  return (int)(nb > cap ? cap : nb < 1 ? 1 : nb);
}

static inline bool aligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ float sq4(const float4& a) { return dot4(a, a); }

// blockDim.x as a kernel reads it.  Inside a device function hipcc does not know that every work-group has the full size and reads
// blockDim.x through a select on the grid's last group.
__device__ __forceinline__ unsigned flat_block_dim() { return __builtin_amdgcn_workgroup_size_x(); }

// This thread's share of a pass over n fp32 elements, two 16-byte vectors per trip: pair(i, j) for the vectors i and j = i + stride
// (elements 4i .. 4i + 3), one(i) for what a thread has left behind its pairs, tail(t) for the n % 4 elements t behind the last
// vector (threads of block 0).  Every element goes to exactly one thread, at any grid size; a pass that writes where it reads (or
// where another of its pointers may point) keeps all reads of a call in front of its writes and leaves __restrict__ off.
template <class Pair, class One, class Tail>
__device__ __forceinline__ void flat_pass2(int64_t n, Pair pair, One one, Tail tail) {
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * flat_block_dim();
  int64_t i = (int64_t)blockIdx.x * flat_block_dim() + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) pair(i, i + stride);
  for (; i < n4; i += stride) one(i);
  if (blockIdx.x == 0 && threadIdx.x < (n - n4 * 4)) tail(n4 * 4 + threadIdx.x);
}

// The same with one vector per trip, for the passes without a second accumulator
template <class One, class Tail>
__device__ __forceinline__ void flat_pass1(int64_t n, One one, Tail tail) {
  const int64_t n4 = n / 4, stride = (int64_t)gridDim.x * flat_block_dim();
  for (int64_t i = (int64_t)blockIdx.x * flat_block_dim() + threadIdx.x; i < n4; i += stride) one(i);
  if (blockIdx.x == 0 && threadIdx.x < (n - n4 * 4)) tail(n4 * 4 + threadIdx.x);
}

// acc[k] = this thread's share of the sum of partial[k * nblk .. (k + 1) * nblk) over a 256-thread block, in double and in index
// order; the K sums of a finish kernel in one loop
template <int K>
__device__ __forceinline__ void fold_partials_f64(const float* __restrict__ partial, int nblk, double (&acc)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += (double)partial[k * nblk + b];
  }
}

// sum of v over a 256-thread block in double, fixed association; valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* sm) {
  __syncthreads();
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
    __syncthreads();
  }
  return sm[0];
}

}  // namespace mafed
