// 8 consecutive elements of a row <-> float[8]: one 16-byte bf16 or two 16-byte fp32 accesses per lane (the coalesced row
// shape of the GEMM epilogues after their LDS pass and of the decode attention's K / V chunks).  p is 16-byte aligned.
#pragma once
#include "common.h"

namespace mafed {

__device__ __forceinline__ void unpack8(const uint4& r, float (&v)[8]) {
  v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
  v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
  v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xffff0000u);
  v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
  uint4 r;
  r.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
  r.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
  r.z = (uint32_t)f32_to_bf16(v[4]) | ((uint32_t)f32_to_bf16(v[5]) << 16);
  r.w = (uint32_t)f32_to_bf16(v[6]) | ((uint32_t)f32_to_bf16(v[7]) << 16);
  return r;
}

__device__ __forceinline__ void load8(const float* __restrict__ p, float (&v)[8]) {
  const float4 a = load4(p), b = load4(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void load8(const bf16_t* __restrict__ p, float (&v)[8]) { unpack8(*reinterpret_cast<const uint4*>(p), v); }
__device__ __forceinline__ void store8(float* __restrict__ p, const float (&v)[8]) {
  store4(p, make_float4(v[0], v[1], v[2], v[3]));
  store4(p + 4, make_float4(v[4], v[5], v[6], v[7]));
}
__device__ __forceinline__ void store8(bf16_t* __restrict__ p, const float (&v)[8]) { *reinterpret_cast<uint4*>(p) = pack8(v); }

// chunk c (8 dims) of a q / k row, rotated for position pos (tf:111-151: NeoX half pairing over the first rot dims); rot % 16 == 0
template <typename T>
__device__ __forceinline__ void load_chunk_rot8(const T* __restrict__ row, int c, int rot, const float* __restrict__ rc, const float* __restrict__ rs,
                                                int pos, float (&o)[8]) {
  load8(row + c * 8, o);
  if (c * 8 >= rot) return;
  const int hc = rot >> 4, half = rot >> 1;
  const bool first = c < hc;
  float y[8];
  load8(row + (first ? c + hc : c - hc) * 8, y);
  const float* cp = rc + (int64_t)pos * half + (first ? c : c - hc) * 8;
  const float* sp = rs + (int64_t)pos * half + (first ? c : c - hc) * 8;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = first ? o[e] * cp[e] - y[e] * sp[e] : o[e] * cp[e] + y[e] * sp[e];
}

}  // namespace mafed
