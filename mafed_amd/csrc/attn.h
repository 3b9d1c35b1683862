// Shared declarations of the attention kernels: exact-fp32 parity kernels (attn_ref.hip), bf16 MFMA kernels (attn_mfma.hip), the
// KV-cached decode kernels (attn_decode.hip), the shared-image prefill's suffix attention and prefix gather (attn_suffix.hip) and the
// candidate attention of model.score (attn_cand.hip).
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

// One exact forward row for one wave (the parity kernels: the full forward, the suffix and the candidate attention).  key(k), for
// k = 0 .. nk - 1 in sequence order, says where the fused q | k | v row of key k is, at which position it rotates and whether the
// query sees it.  qrow[D] holds the rotated query, sc[nk] is scratch (both LDS of this wave); writes softmax(q K^T / sqrt D) V to
// op[D] and returns the row's maximum and sum through m, l.
template <typename T>
struct AttnKey {
  const T* row;
  int pos;
  bool visible;
};
template <typename T, typename Key>
__device__ __forceinline__ void attn_exact_row(const float* __restrict__ qrow, float* __restrict__ sc, int nk, int D, int rot,
                                               const float* __restrict__ rc, const float* __restrict__ rs, Key key, T* __restrict__ op,
                                               int lane, float& m, float& l) {
  const int half = rot >> 1;
  const float scale = rsqrtf((float)D);
  m = -INFINITY;
  for (int k = lane; k < nk; k += 64) {
    float s = -INFINITY;
    const AttnKey<T> kk = key(k);
    if (kk.visible) {
      float acc = 0.f;
      for (int d = 0; d < D; ++d)
        acc = fmaf(qrow[d], rot_elem(kk.row + D, d, rot, rc + (int64_t)kk.pos * half, rs + (int64_t)kk.pos * half), acc);
      s = acc * scale;
    }
    sc[k] = s;
    m = fmaxf(m, s);
  }
  m = wave_max(m);
  l = 0.f;
  for (int k = lane; k < nk; k += 64) {
    const float p = expf(sc[k] - m);
    sc[k] = p;
    l += p;
  }
  l = wave_sum(l);
  __builtin_amdgcn_wave_barrier();
  const float inv = 1.0f / l;
  for (int d = lane; d < D; d += 64) {
    float acc = 0.f;
    for (int k = 0; k < nk; ++k) acc = fmaf(sc[k], Elem<T>::load(key(k).row + 2 * D + d), acc);
    Elem<T>::store(op + d, acc * inv);
  }
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

// Suffix attention (attn_suffix.hip, attn_mfma.hip): the T text queries of prompt b against the P keys of image image_index[b] (NULL:
// image b) followed by the prompt's own text keys = rows P .. P+T-1 of the forward above on the assembled [B, P+T] sequence.
struct SuffixShape {
  int B, N, P, T, H, D, rot;
};
// image of prompt b, clamped into [0, N): the host validates the index, a stray value must still not leave the image store
__device__ __forceinline__ int64_t suffix_image(const int64_t* __restrict__ image_index, int b, int N) {
  const int64_t n = image_index ? image_index[b] : (int64_t)b;
  return n < 0 ? 0 : (n >= N ? N - 1 : n);
}
template <typename T>
int attn_suffix_ref_launch(const void* qkv_img, const int64_t* image_index, const void* qkv_txt, const SuffixShape& sh, const float* rc,
                           const float* rs, const int64_t* am, void* out, hipStream_t st);
int attn_suffix_mfma_launch(const void* qkv_img, const int64_t* image_index, const void* qkv_txt, const SuffixShape& sh, const float* rc,
                            const float* rs, const int64_t* am, void* out, hipStream_t st);
// out [L, B*(P+T), W] = per prompt the P rows of its image from img [L, N*P, W], then its T rows from txt [L, B*T, W]
int prefix_gather_launch(const void* img, const void* txt, const int64_t* image_index, int L, int N, int B, int P, int T, int64_t row_bytes,
                         void* out, hipStream_t st);

// Candidate attention (attn_cand.hip, attn_mfma.hip): the A rows of each of the C candidates of prompt b against the prompt's S0 prefix
// keys (P = S0 - T image keys, T left-padded text keys) followed by the candidate's own earlier rows = rows S0 .. S0+A-1 of the forward
// above on every assembled [prefix b | candidate (b, c)] sequence.
struct CandShape {
  int B, C, A, S0, T, H, D, rot;
};
template <typename T>
int attn_cand_ref_launch(const void* qkv_pre, const void* qkv_cand, const CandShape& sh, const float* rc, const float* rs, const int64_t* am,
                         void* out, hipStream_t st);
int attn_cand_mfma_launch(const void* qkv_pre, const void* qkv_cand, const CandShape& sh, const float* rc, const float* rs, const int64_t* am,
                          void* out, hipStream_t st);

void attn_mfma_set_variant(int v);  // 0 automatic (resident kernels when K/V fit in LDS), 1 tiled kernels only

int attn_decode_set_trace(void* buf);   // tools: [B * H][8] stamps of the next flat decode attention launches

}  // namespace mafed
