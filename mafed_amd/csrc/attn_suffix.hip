// Shared-image prefill (generate / sample with image_index; DESIGN.md section 4c'''): the exact suffix attention and the prefix gather.
// The prompt is [P image tokens | T text tokens], fully causal, positions arange: the K and V of the image rows depend on the image
// alone, so they are computed once per distinct image into an image store [N, P, H, 3, D] and the text rows of every prompt attend
// them through image_index.  Suffix attention = rows P .. P+T-1 of mafed_attn_fwd on the assembled [B, P+T] sequence: query j of
// prompt b sits at position P + j and sees the P keys of image image_index[b] and the text keys 0 .. j of its own prompt that the
// left-padding mask leaves; rotary on load with position = key index; softmax in fp32.  A query at a padded position (or of an
// all-padding prompt) still sees the image keys, as the full forward's rows do.
// This file: the exact kernel (fp32 parity mode; bf16 head sizes without an MFMA kernel) one wave per query row: a shell
// around the exact forward row it shares with attn_ref.hip (attn.h, attn_exact_row), which it tells where key j lives.  The bf16 MFMA
// kernel lives beside the tiled forward and shares its tile step (attn_mfma.hip, attn_suffix_mfma_kernel).
#include "attn.h"

namespace mafed {

// LDS per wave: qrow[D] + sc[P + T] floats
template <typename T>
__global__ __launch_bounds__(256) void attn_suffix_ref_kernel(const T* __restrict__ qkv_img, const int64_t* __restrict__ image_index,
                                                              const T* __restrict__ qkv_txt, SuffixShape sh, const float* __restrict__ rc,
                                                              const float* __restrict__ rs, const int64_t* __restrict__ am,
                                                              T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int P = sh.P, Tt = sh.T, H = sh.H, D = sh.D, rot = sh.rot, half = sh.rot >> 1;
  const int q = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
  float* qrow = lds + (size_t)wave * (D + P + Tt);
  float* sc = qrow + D;
  if (q >= Tt) return;
  const int64_t rstride = (int64_t)H * 3 * D;
  const T* ib = qkv_img + (suffix_image(image_index, b, sh.N) * P * H + h) * 3 * D;  // + j * rstride + {0, D, 2D}
  const T* tb = qkv_txt + ((int64_t)b * Tt * H + h) * 3 * D;
  const int pos = P + q;
  for (int d = lane; d < D; d += 64) qrow[d] = rot_elem(tb + (int64_t)q * rstride, d, rot, rc + (int64_t)pos * half, rs + (int64_t)pos * half);
  __builtin_amdgcn_wave_barrier();
  float m, l;
  attn_exact_row(qrow, sc, pos + 1, D, rot, rc, rs,
                 [&](int j) {
                   return AttnKey<T>{j < P ? ib + (int64_t)j * rstride : tb + (int64_t)(j - P) * rstride, j, key_valid(am, b, j, P, Tt)};
                 },
                 out + ((int64_t)b * Tt + q) * H * D + (int64_t)h * D, lane, m, l);
}

template <typename T>
int attn_suffix_ref_launch(const void* qkv_img, const int64_t* image_index, const void* qkv_txt, const SuffixShape& sh, const float* rc,
                           const float* rs, const int64_t* am, void* out, hipStream_t st) {
  const size_t lds = (size_t)4 * (sh.D + sh.P + sh.T) * sizeof(float);
  if (lds > 160 * 1024) { set_error("attn_suffix_fwd: P+T=%d too long for the exact kernel", sh.P + sh.T); return MAFED_EINVAL; }
  auto k = attn_suffix_ref_kernel<T>;
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  k<<<dim3((sh.T + 3) / 4, sh.H, sh.B), dim3(256), lds, st>>>((const T*)qkv_img, image_index, (const T*)qkv_txt, sh, rc, rs, am, (T*)out);
  return MAFED_OK;
}

template int attn_suffix_ref_launch<float>(const void*, const int64_t*, const void*, const SuffixShape&, const float*, const float*,
                                           const int64_t*, void*, hipStream_t);
template int attn_suffix_ref_launch<bf16_t>(const void*, const int64_t*, const void*, const SuffixShape&, const float*, const float*,
                                            const int64_t*, void*, hipStream_t);

// Prefix assembly for the decode cache: one block per output row (layer l, prompt b, position s), a plain 16-byte-per-lane copy of
// the row from the image store (s < P: row image_index[b] * P + s of layer l) or from the text store (row b * T + s - P).
__global__ __launch_bounds__(256) void prefix_gather_kernel(const uint4* __restrict__ img, const uint4* __restrict__ txt,
                                                            const int64_t* __restrict__ image_index, int N, int B, int P, int T, int chunks,
                                                            uint4* __restrict__ out) {
  const int S0 = P + T;
  const int64_t row = blockIdx.x;   // (l * B + b) * S0 + s
  const int s = (int)(row % S0);
  const int64_t lb = row / S0;
  const int b = (int)(lb % B);
  const int64_t l = lb / B;
  const uint4* src = s < P ? img + ((l * N + suffix_image(image_index, b, N)) * P + s) * chunks
                           : txt + ((l * B + b) * T + (s - P)) * chunks;
  uint4* dst = out + row * chunks;
  for (int c = threadIdx.x; c < chunks; c += 256) dst[c] = src[c];
}

int prefix_gather_launch(const void* img, const void* txt, const int64_t* image_index, int L, int N, int B, int P, int T, int64_t row_bytes,
                         void* out, hipStream_t st) {
  const int64_t rows = (int64_t)L * B * (P + T);
  if (rows > 0x7fffffffLL || row_bytes % 16 != 0 || row_bytes / 16 > 0x7fffffffLL) {
    set_error("prefix_gather: %lld rows of %lld bytes (rows must be a multiple of 16 bytes)", (long long)rows, (long long)row_bytes);
    return MAFED_EINVAL;
  }
  prefix_gather_kernel<<<dim3((unsigned)rows), dim3(256), 0, st>>>((const uint4*)img, (const uint4*)txt, image_index, N, B, P, T,
                                                                    (int)(row_bytes / 16), (uint4*)out);
  return MAFED_OK;
}

}  // namespace mafed
