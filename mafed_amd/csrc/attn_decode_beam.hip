// Decode attention for the k beams of a sample (model.generate(num_beams=k); candidates and bookkeeping: beam.hip), the fourth kernel
// of attn_decode.hip's table -- a file of its own only because the fused kernels' code depends on what else calls load_chunk_rot8 in
// their translation unit (see there).
// Cache layout: per layer the prefix [B, S0, 3*H*D] (pre-rotated keys, written by one prefill per sample) and the generated rows
// [B*k, cap, 3*H*D]; beam slot r writes its row t at [r, t] and never moves it.  anc[r, j] (int32, global slot index) names the slot
// that holds row j of beam r's history; a reorder rewrites anc only, so no K/V is copied.
#include "common.h"
#include "row8.h"

namespace mafed {

// online-softmax state (m, l, acc) += one key row (score s, value chunk v)
__device__ __forceinline__ void online_add(float& m, float& l, float (&acc)[8], float s, const float (&v)[8]) {
  const float mn = fmaxf(m, s);
  const float corr = m == -INFINITY ? 0.f : __expf(m - mn);
  const float p = __expf(s - mn);
  l = l * corr + p;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = fmaf(acc[e], corr, p * v[e]);
  m = mn;
}

// Grid (H, B), 256 threads.  Thread (key group kg, chunk c) takes 16-byte chunk c of k and of v of a key row; UNR rows in flight.
// Prefix rows: each loaded once and scored against all k queries (k online-softmax states per thread).  Generated rows: (beam, row)
// pairs spread over the key groups; row j < t of beam r comes from slot anc[r, j], row t from the beam's own slot (its key rotated
// here, used from LDS and written back rotated for the later steps: this block is the only user of row t's (b, h) slices).  The
// states are merged over the key groups with shuffles inside a wave and through LDS across the four waves.
template <typename T, int D, int KB>
__global__ __launch_bounds__(256) void attn_decode_beam_kernel(const T* __restrict__ qkv_pre, int S0, T* __restrict__ qkv_new, int cap, int t,
                                                               int k, const int* __restrict__ anc, int H, int rot, int P, int Tm,
                                                               const float* __restrict__ rc, const float* __restrict__ rs,
                                                               const int64_t* __restrict__ am, T* __restrict__ out) {
  constexpr int chunks = D / 8, groups = 256 / chunks, UNR = 4;
  __shared__ float q_s[KB][D];
  __shared__ float knew_s[KB][D];
  __shared__ float red[4][KB][D];
  __shared__ float ml[4][KB][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, b = blockIdx.y;
  const int64_t rstride = (int64_t)H * 3 * D;
  const T* pre = qkv_pre + ((int64_t)b * S0 * H + h) * 3 * D;
  T* neu = qkv_new + (int64_t)h * 3 * D;   // row j of slot s at neu + (s * cap + j) * rstride
  const int64_t slot0 = (int64_t)b * k;
  const int c = tid % chunks, kg = tid / chunks;
  const float scale = rsqrtf((float)D);
  for (int idx = tid; idx < k * chunks; idx += 256) {
    const int r = idx / chunks, cc = idx - r * chunks;
    const T* row = neu + ((slot0 + r) * cap + t) * rstride;
    float v[8];
    load_chunk_rot8<T>(row, cc, rot, rc, rs, S0 + t, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) q_s[r][cc * 8 + e] = v[e] * scale;
    load_chunk_rot8<T>(row + D, cc, rot, rc, rs, S0 + t, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) knew_s[r][cc * 8 + e] = v[e];
  }
  __syncthreads();
  for (int idx = tid; idx < k * chunks; idx += 256) {   // every read of the un-rotated key is behind the barrier
    const int r = idx / chunks, cc = idx - r * chunks;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = knew_s[r][cc * 8 + e];
    store8(neu + ((slot0 + r) * cap + t) * rstride + D + cc * 8, v);
  }
  float qr[KB][8], m[KB], l[KB], acc[KB][8];
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      qr[r][e] = r < k ? q_s[r][c * 8 + e] : 0.f;
      acc[r][e] = 0.f;
    }
  }
  // the prefix: shared by the k beams, every row loaded once
  for (int j0 = 0; j0 < S0; j0 += UNR * groups) {
    float kx[UNR][8], vx[UNR][8];
    int64_t mw[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {   // unconditional clamped loads, all in flight before the first use
      const int j = j0 + u * groups + kg;
      const int jc = j < S0 ? j : S0 - 1;
      const T* row = pre + (int64_t)jc * rstride;
      load8(row + D + c * 8, kx[u]);
      load8(row + 2 * D + c * 8, vx[u]);
      mw[u] = am[(int64_t)b * Tm + (jc >= P ? jc - P : 0)];
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * groups + kg;
      const bool ok = j < S0 && (j < P || mw[u] != 0);
#pragma unroll
      for (int r = 0; r < KB; ++r) {
        if (r < k) {
          float s = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) s = fmaf(qr[r][e], kx[u][e], s);
#pragma unroll
          for (int o = 1; o < chunks; o <<= 1) s += __shfl_xor(s, o, 64);
          if (ok) online_add(m[r], l[r], acc[r], s, vx[u]);
        }
      }
    }
  }
  // the generated rows: (beam r, row j <= t) pairs
  const int npairs = k * (t + 1);
  for (int q0 = 0; q0 < npairs; q0 += groups) {
    const int q = q0 + kg;
    const bool ok = q < npairs;
    const int qc = ok ? q : 0;
    const int r = qc / (t + 1), j = qc - r * (t + 1);
    const bool own = j == t;
    const int64_t slot = own ? slot0 + r : (int64_t)anc[(slot0 + r) * cap + j];
    const T* row = neu + (slot * cap + j) * rstride;
    float kx[8], vx[8];
    load8(row + D + c * 8, kx);
    load8(row + 2 * D + c * 8, vx);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(q_s[r][c * 8 + e], own ? knew_s[r][c * 8 + e] : kx[e], s);
#pragma unroll
    for (int o = 1; o < chunks; o <<= 1) s += __shfl_xor(s, o, 64);
#pragma unroll
    for (int rr = 0; rr < KB; ++rr)
      if (ok && rr == r) online_add(m[rr], l[rr], acc[rr], s, vx);
  }
  // merge the key groups: shuffles inside the wave, then LDS across the waves
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    if (r < k) {
#pragma unroll
      for (int o = chunks; o < 64; o <<= 1) {
        const float m2 = __shfl_xor(m[r], o, 64), l2 = __shfl_xor(l[r], o, 64);
        const float mn = fmaxf(m[r], m2);
        const float w1 = m[r] == -INFINITY ? 0.f : __expf(m[r] - mn), w2 = m2 == -INFINITY ? 0.f : __expf(m2 - mn);
        l[r] = l[r] * w1 + l2 * w2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float a2 = __shfl_xor(acc[r][e], o, 64);
          acc[r][e] = acc[r][e] * w1 + a2 * w2;
        }
        m[r] = mn;
      }
      if (lane < chunks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wave][r][c * 8 + e] = acc[r][e];
        if (lane == 0) { ml[wave][r][0] = m[r]; ml[wave][r][1] = l[r]; }
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < k * D; idx += 256) {
    const int r = idx / D, d = idx - r * D;
    float mx = ml[0][r][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) mx = fmaxf(mx, ml[w][r][0]);
    float o = 0.f, lt = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float wt = ml[w][r][0] == -INFINITY ? 0.f : __expf(ml[w][r][0] - mx);
      o = fmaf(wt, red[w][r][d], o);
      lt = fmaf(wt, ml[w][r][1], lt);
    }
    Elem<T>::store(out + (slot0 + r) * H * D + (int64_t)h * D + d, lt > 0.f ? o / lt : 0.f);
  }
}

template <typename T, int D>
void attn_decode_beam_go(const void* pre, int S0, void* neu, int cap, int t, int B, int k, const int* anc, int H, int rot, int P, int Tm,
                         const float* rc, const float* rs, const int64_t* am, void* out, hipStream_t st) {
  const dim3 grid(H, B), block(256);
#define GO(KBV) attn_decode_beam_kernel<T, D, KBV><<<grid, block, 0, st>>>((const T*)pre, S0, (T*)neu, cap, t, k, anc, H, rot, P, Tm, rc, rs, am, (T*)out)
  if (k <= 2) GO(2);
  else if (k <= 4) GO(4);
  else GO(8);
#undef GO
}

}  // namespace mafed

using namespace mafed;

extern "C" int mafed_attn_decode_beam(const void* qkv_prefix, int S0, void* qkv_new, int cap, int t, mafed_dtype dtype, int B, int k,
                                      const int* anc, int H, int D, int rot, const float* rot_cos, const float* rot_sin,
                                      const int64_t* attention_mask, int T, void* out, void* stream) {
  MAFED_CHECK_ARG(qkv_prefix && qkv_new && anc && out && attention_mask && rot_cos && rot_sin, "attn_decode_beam: null pointer");
  MAFED_CHECK_ARG(B > 0 && k >= 1 && k <= 8 && H > 0 && (D == 64 || D == 128 || D == 256) && S0 > 0 && T >= 1 && T <= S0 && cap > 0 && t >= 0 &&
                  t < cap, "attn_decode_beam: bad shape B=%d k=%d H=%d D=%d S0=%d T=%d cap=%d t=%d", B, k, H, D, S0, T, cap, t);
  MAFED_CHECK_ARG(rot > 0 && rot <= D && rot % 16 == 0, "attn_decode_beam: needs a pre-rotated cache (rot %% 16 == 0)");
  hipStream_t st = as_stream(stream);
  const int P = S0 - T;
  if (dtype == MAFED_F32) {
    if (D == 64) attn_decode_beam_go<float, 64>(qkv_prefix, S0, qkv_new, cap, t, B, k, anc, H, rot, P, T, rot_cos, rot_sin, attention_mask, out, st);
    else if (D == 128) attn_decode_beam_go<float, 128>(qkv_prefix, S0, qkv_new, cap, t, B, k, anc, H, rot, P, T, rot_cos, rot_sin, attention_mask, out, st);
    else attn_decode_beam_go<float, 256>(qkv_prefix, S0, qkv_new, cap, t, B, k, anc, H, rot, P, T, rot_cos, rot_sin, attention_mask, out, st);
  } else {
    if (D == 64) attn_decode_beam_go<bf16_t, 64>(qkv_prefix, S0, qkv_new, cap, t, B, k, anc, H, rot, P, T, rot_cos, rot_sin, attention_mask, out, st);
    else if (D == 128) attn_decode_beam_go<bf16_t, 128>(qkv_prefix, S0, qkv_new, cap, t, B, k, anc, H, rot, P, T, rot_cos, rot_sin, attention_mask, out, st);
    else attn_decode_beam_go<bf16_t, 256>(qkv_prefix, S0, qkv_new, cap, t, B, k, anc, H, rot, P, T, rot_cos, rot_sin, attention_mask, out, st);
  }
  MAFED_CHECK_LAUNCH("attn_decode_beam");
  return MAFED_OK;
}