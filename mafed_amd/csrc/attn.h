// Shared declarations of the attention kernels: exact-fp32 parity kernels (attn_ref.hip), bf16 MFMA kernels (attn_mfma.hip) and the
// KV-cached decode kernels (attn_decode.hip).
#pragma once
#include "common.h"

namespace mafed {

struct AttnShape {
  int B, S, H, D, rot, T, P;
  int causal = 1;  // 0: bidirectional (the frozen CLIP vision tower, forward only)
};

// scalar forms shared by the parity kernels and the wave-per-head decode kernel
// element d of the rotated row (tf:111-151): first `rot` dims rotate with the NeoX half pairing d <-> d +- rot/2
template <typename T>
__device__ __forceinline__ float rot_elem(const T* __restrict__ row, int d, int rot, const float* __restrict__ c, const float* __restrict__ s) {
  const float x = Elem<T>::load(row + d);
  if (d >= rot) return x;
  const int half = rot >> 1;
  if (d < half) return x * c[d] - Elem<T>::load(row + d + half) * s[d];
  return x * c[d - half] + Elem<T>::load(row + d - half) * s[d - half];
}
__device__ __forceinline__ bool key_valid(const int64_t* __restrict__ am, int b, int j, int P, int T) {
  return j < P || am[(int64_t)b * T + (j - P)] != 0;
}

template <typename T>
int attn_ref_fwd_launch(const void* qkv, const AttnShape& sh, const float* rc, const float* rs, const int64_t* am, void* out, float* lse,
                        hipStream_t st);
template <typename T>
int attn_ref_bwd_launch(const void* qkv, const void* out, const void* dout, const float* lse, const AttnShape& sh, const float* rc,
                        const float* rs, const int64_t* am, void* dqkv, float* delta, hipStream_t st);

template <typename T>
int attn_decode_launch(const void* qkv_pre, int S0, const void* qkv_new, int cap, int t, int B, int H, int D, int rot, int P, int Tm,
                       const float* rc, const float* rs, const int64_t* am, void* out, hipStream_t st, bool prerot = false);
// k part of every row of a [rows / S samples, S, H, 3, D] qkv tensor rotated in place for its position (decode cache)
template <typename T>
int rotate_k_rows_launch(void* qkv, int64_t rows, int S, int H, int D, int rot, const float* rc, const float* rs, hipStream_t st);

int attn_mfma_fwd_launch(const void* qkv, const AttnShape& sh, const float* rc, const float* rs, const int64_t* am, void* out, float* lse,
                         hipStream_t st);
int attn_mfma_bwd_launch(const void* qkv, const void* out, const void* dout, const float* lse, const AttnShape& sh, const float* rc,
                         const float* rs, const int64_t* am, void* dqkv, float* delta, float* colsum, bool* colsum_done, hipStream_t st);

void attn_mfma_set_variant(int v);  // 0 automatic (resident kernels when K/V fit in LDS), 1 tiled kernels only

int attn_decode_set_trace(void* buf);   // tools: [B * H][8] stamps of the next flat decode attention launches

}  // namespace mafed
