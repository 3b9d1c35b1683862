// Candidate attention (model.score; DESIGN.md section 4c''''): C candidate answers of A tokens each behind ONE prefilled prompt.
// The prompt's fused-QKV rows [B, S0, H, 3, D] (S0 = P image + T left-padded text positions, keys un-rotated, as the QKV GEMM wrote
// them) are the prefix; the candidates' rows are [B, C, A, H, 3, D].  Row (b, c, j) equals row S0 + j of mafed_attn_fwd on the assembled
// sequence [prefix b | candidate (b, c)] of length S0 + A under the mask [attention_mask[b] | ones(A)]: the query sits at position
// S0 + j and sees the P image keys, the prefix text keys the padding mask leaves and keys 0 .. j of its OWN candidate -- nothing of
// another candidate; rotary on load with position = key index (candidate key j' is at S0 + j' for every c); softmax in fp32.  Every
// query sees key 0 (an image key: P >= 1), so no row is empty, whatever the text mask.
// This file: the exact kernel (fp32 parity mode; bf16 head sizes without an MFMA kernel) one wave per query row: a shell
// around the exact forward row it shares with attn_ref.hip (attn.h, attn_exact_row), which it tells where key k lives.  The bf16 MFMA
// kernel lives beside the tiled forward and shares its tile step (attn_mfma.hip, attn_cand_mfma_kernel).
#include "attn.h"

namespace mafed {

// LDS per wave: qrow[D] + sc[S0 + A] floats
template <typename T>
__global__ __launch_bounds__(256) void attn_cand_ref_kernel(const T* __restrict__ qkv_pre, const T* __restrict__ qkv_cand, CandShape sh,
                                                            const float* __restrict__ rc, const float* __restrict__ rs,
                                                            const int64_t* __restrict__ am, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S0 = sh.S0, Tt = sh.T, P = sh.S0 - sh.T, A = sh.A, CA = sh.C * sh.A, H = sh.H, D = sh.D, rot = sh.rot, half = sh.rot >> 1;
  const int r = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;   // r = c * A + j
  float* qrow = lds + (size_t)wave * (D + S0 + A);
  float* sc = qrow + D;
  if (r >= CA) return;
  const int j = r % A;
  const int64_t rstride = (int64_t)H * 3 * D;
  const T* pb = qkv_pre + ((int64_t)b * S0 * H + h) * 3 * D;                     // + key * rstride + {0, D, 2D}
  const T* cb = qkv_cand + (((int64_t)b * CA + (r - j)) * H + h) * 3 * D;        // row 0 of this query's candidate
  const int pos = S0 + j, nk = pos + 1;                                         // keys 0 .. S0 - 1 of the prefix, S0 .. S0 + j of the candidate
  for (int d = lane; d < D; d += 64) qrow[d] = rot_elem(cb + (int64_t)j * rstride, d, rot, rc + (int64_t)pos * half, rs + (int64_t)pos * half);
  __builtin_amdgcn_wave_barrier();
  float m, l;
  attn_exact_row(qrow, sc, nk, D, rot, rc, rs,
                 [&](int k) {
                   return AttnKey<T>{k < S0 ? pb + (int64_t)k * rstride : cb + (int64_t)(k - S0) * rstride, k,
                                     k >= S0 || key_valid(am, b, k, P, Tt)};
                 },
                 out + ((int64_t)b * CA + r) * H * D + (int64_t)h * D, lane, m, l);
}

template <typename T>
int attn_cand_ref_launch(const void* qkv_pre, const void* qkv_cand, const CandShape& sh, const float* rc, const float* rs, const int64_t* am,
                         void* out, hipStream_t st) {
  const size_t lds = (size_t)4 * (sh.D + sh.S0 + sh.A) * sizeof(float);
  if (lds > 160 * 1024) { set_error("attn_cand_fwd: S0+A=%d too long for the exact kernel", sh.S0 + sh.A); return MAFED_EINVAL; }
  auto k = attn_cand_ref_kernel<T>;
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  k<<<dim3((sh.C * sh.A + 3) / 4, sh.H, sh.B), dim3(256), lds, st>>>((const T*)qkv_pre, (const T*)qkv_cand, sh, rc, rs, am, (T*)out);
  return MAFED_OK;
}

template int attn_cand_ref_launch<float>(const void*, const void*, const CandShape&, const float*, const float*, const int64_t*, void*,
                                         hipStream_t);
template int attn_cand_ref_launch<bf16_t>(const void*, const void*, const CandShape&, const float*, const float*, const int64_t*, void*,
                                          hipStream_t);

}  // namespace mafed
