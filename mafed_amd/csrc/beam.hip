// Beam search over a shared-prefix KV cache (model.generate(num_beams=k); HF GenerationMixin._beam_search semantics, transformers 5.x):
//
//   a  beam_candidates   per sample, the top 2k of log_softmax(logits[row]) + score[row] over its kin rows x V tokens
//   b  beam_update       per sample, HF's bookkeeping on the device: finished hypotheses (top k by length-normalised score), the
//                        early-stopping flag, the k continuing beams (parent, token, score) and the ancestry / token-history rewrite
//
// The decode attention of the k beams reads the ancestry table this file maintains (attn_decode.hip: attn_decode_beam_kernel, which
// also documents the cache layout): a reorder rewrites anc only (anc'[r, j] = anc[parent(r), j] for j < t, anc'[r, t] = r).
#include "common.h"

namespace mafed {
namespace {

// ---- a: candidates ----------------------------------------------------------------------------------------------------------------
// Order: score descending, ties to the lower flat index beam * V + token.  Both as ONE 64-bit unsigned key compared with `>`: high
// word = order-preserving image of the fp32 score, low word = 0xffffffff - flat.  Keys are unique (flat indices are); 0 is below all.
__device__ __forceinline__ uint32_t ord_f32(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f32(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

template <typename T>
__device__ __forceinline__ float ld1(const T* p);
template <>
__device__ __forceinline__ float ld1<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ld1<bf16_t>(const bf16_t* p) { return bf16_to_f32(*p); }

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}

constexpr int CAND_NT = 512, CAND_U = 8;   // threads per sample, loads in flight per thread

// One workgroup per sample.  Pass 1, per row: max and sum of exp (online per thread, merged over the block) -> max + log(sum).
// Pass 2: every element's log-probability + row score goes into the thread's register-resident sorted top-K2 (a compare-swap chain,
// entered only by an element that beats the thread's current K2-th key).  Then K2 rounds of a block-wide argmax over the list heads.
template <typename T, int K2>
__global__ __launch_bounds__(CAND_NT) void beam_candidates_kernel(const T* __restrict__ logits, int64_t ldl, const float* __restrict__ score,
                                                                 int kin, int V, float* __restrict__ out_score, int64_t* __restrict__ out_tok,
                                                                 int* __restrict__ out_par) {
  constexpr int NW = CAND_NT / 64;
  __shared__ float s_m[NW], s_l[NW];
  __shared__ float row_sub[8];   // max + log(sum exp) per row (kin <= 8)
  __shared__ unsigned long long s_key[NW];
  __shared__ unsigned long long s_sel[K2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  for (int r = 0; r < kin; ++r) {
    const T* row = logits + (int64_t)(b * kin + r) * ldl;
    float m = -INFINITY, l = 0.f;
    for (int i0 = tid; i0 < V; i0 += CAND_NT * CAND_U) {
      float xs[CAND_U];
#pragma unroll
      for (int u = 0; u < CAND_U; ++u) {   // CAND_U loads in flight per thread (clamped index; the tail is skipped below)
        const int i = i0 + u * CAND_NT;
        xs[u] = ld1<T>(row + (i < V ? i : V - 1));
      }
#pragma unroll
      for (int u = 0; u < CAND_U; ++u) {
        if (i0 + u * CAND_NT >= V) break;
        const float x = xs[u];
        if (x > m) {
          l = l * __expf(m - x) + 1.f;
          m = x;
        } else {
          l += __expf(x - m);
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
      const float mn = fmaxf(m, m2);
      l = (m == -INFINITY ? 0.f : l * __expf(m - mn)) + (m2 == -INFINITY ? 0.f : l2 * __expf(m2 - mn));
      m = mn;
    }
    if (lane == 0) { s_m[wave] = m; s_l[wave] = l; }
    __syncthreads();
    if (tid == 0) {
      float mx = s_m[0];
      for (int w = 1; w < NW; ++w) mx = fmaxf(mx, s_m[w]);
      float sum = 0.f;
      for (int w = 0; w < NW; ++w) sum += s_m[w] == -INFINITY ? 0.f : s_l[w] * expf(s_m[w] - mx);
      row_sub[r] = mx + logf(sum);
    }
    __syncthreads();
  }
  unsigned long long lst[K2];
#pragma unroll
  for (int j = 0; j < K2; ++j) lst[j] = 0ull;
  for (int r = 0; r < kin; ++r) {
    const T* row = logits + (int64_t)(b * kin + r) * ldl;
    const float sub = row_sub[r], sc = score[b * kin + r];
    const uint32_t base = 0xffffffffu - (uint32_t)(r * V);
    for (int i0 = tid; i0 < V; i0 += CAND_NT * CAND_U) {
      float xs[CAND_U];
#pragma unroll
      for (int u = 0; u < CAND_U; ++u) {
        const int i = i0 + u * CAND_NT;
        xs[u] = ld1<T>(row + (i < V ? i : V - 1));
      }
#pragma unroll
      for (int u = 0; u < CAND_U; ++u) {
        const int i = i0 + u * CAND_NT;
        if (i >= V) break;
        const float v = (xs[u] - sub) + sc;
        unsigned long long key = ((unsigned long long)ord_f32(v) << 32) | (unsigned long long)(base - (uint32_t)i);
        if (key > lst[K2 - 1]) {
#pragma unroll
          for (int j = 0; j < K2; ++j) {
            const unsigned long long a = lst[j];
            const bool gt = key > a;
            lst[j] = gt ? key : a;
            key = gt ? a : key;
          }
        }
      }
    }
  }
  for (int s = 0; s < K2; ++s) {
    unsigned long long best = lst[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = shfl_xor_u64(best, o);
      best = other > best ? other : best;
    }
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    best = s_key[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) best = s_key[w] > best ? s_key[w] : best;
    if (lst[0] == best) {   // exactly one thread holds it (keys are unique): pop its head
#pragma unroll
      for (int j = 0; j < K2 - 1; ++j) lst[j] = lst[j + 1];
      lst[K2 - 1] = 0ull;
    }
    if (tid == 0) s_sel[s] = best;
    __syncthreads();   // s_key is rewritten by the next round
  }
  if (tid < K2) {
    const unsigned long long key = s_sel[tid];
    const uint32_t flat = 0xffffffffu - (uint32_t)key;
    out_score[b * K2 + tid] = unord_f32((uint32_t)(key >> 32));
    out_tok[b * K2 + tid] = (int64_t)(flat % (uint32_t)V);
    out_par[b * K2 + tid] = (int)(flat / (uint32_t)V);
  }
}

// ---- b: bookkeeping ----------------------------------------------------------------------------------------------------------------
struct BeamUpdateArgs {
  const float* cs;          // [B][2k] candidate scores, best first (beam_candidates)
  const int64_t* ct;        // [B][2k] candidate tokens
  const int* cp;            // [B][2k] candidate parent (beam within the sample)
  int k, n, cap, eos, pad, early;   // n: this step (0-based); cap = max_new_tokens; eos < 0: none; early: 0 False, 1 True, 2 "never"
  float lp;                 // length_penalty
  float* run_score;         // [B*k] running beam scores (written)
  const int* anc_in;        // [B*k][cap] ancestry before the step / after it
  int* anc_out;
  const int64_t* hist_in;   // [B*k][cap] generated tokens of the running beams, before / after
  int64_t* hist_out;
  const int64_t* fin_tok_in;   // [B][k][cap] finished hypotheses (pad beyond their length), best first, before / after
  int64_t* fin_tok_out;
  const float* fin_score_in;   // [B][k] normalised scores (-1e9: empty slot)
  float* fin_score_out;
  const int* fin_len_in;       // [B][k] generated length (0: empty slot)
  int* fin_len_out;
  int* done;                // [B] the sample can no longer change its finished set
  int64_t* next_tok;        // [B*k] the token each beam slot feeds into the next decode step
};

// One wave per sample: lane 0 takes the decisions (k <= 8: a handful of scalar steps), the wave then rewrites the rows.
__global__ __launch_bounds__(64) void beam_update_kernel(BeamUpdateArgs a) {
  __shared__ int s_par[8], s_src[8];
  __shared__ int64_t s_tok[8];
  const int b = blockIdx.x, tid = threadIdx.x, k = a.k, cap = a.cap, n = a.n, k2 = 2 * k;
  const float* cs = a.cs + b * k2;
  const int64_t* ct = a.ct + b * k2;
  const int* cp = a.cp + b * k2;
  if (tid == 0) {
    const bool last = n == cap - 1;   // max_new_tokens reached: every candidate hits a stopping criterion
    const int done = a.done[b];
    int nfin = 0;
    for (int i = 0; i < k; ++i) nfin += a.fin_len_in[b * k + i] > 0;
    const bool add = !done && !(a.early == 1 && nfin == k);
    const float norm = (float)pow((double)(n + 1), (double)a.lp);
    // finished set: the k old entries, then the just-finished candidates among the first k ranks (src >= k: candidate src - k); the k
    // best are kept, best first, earlier entries first on equal scores
    float msc[16];
    int msrc[16], cnt = 0;
    for (int i = 0; i < k; ++i) { msc[cnt] = a.fin_score_in[b * k + i]; msrc[cnt++] = i; }
    if (add)
      for (int i = 0; i < k; ++i)
        if (last || (a.eos >= 0 && ct[i] == a.eos)) { msc[cnt] = cs[i] / norm; msrc[cnt++] = k + i; }
    unsigned used = 0u;
    float worst = 0.f;
    bool all_fin = true;
    for (int s = 0; s < k; ++s) {
      int bi = -1;
      for (int i = 0; i < cnt; ++i)
        if (!(used >> i & 1u) && (bi < 0 || msc[i] > msc[bi])) bi = i;
      used |= 1u << bi;
      const int src = msrc[bi];
      const int len = src < k ? a.fin_len_in[b * k + src] : n + 1;
      s_src[s] = src;
      a.fin_score_out[b * k + s] = msc[bi];
      a.fin_len_out[b * k + s] = len;
      all_fin = all_fin && len > 0;
      worst = s == 0 ? msc[bi] : fminf(worst, msc[bi]);
    }
    // continuing beams: the first k candidates that did not just hit a stopping criterion (all of them on the last step); a sample
    // whose result is final idles on the pad token in place
    float best_run = 0.f;
    if (done) {
      for (int r = 0; r < k; ++r) { s_par[r] = r; s_tok[r] = a.pad; }
    } else {
      int nr = 0;
      for (int i = 0; i < k2 && nr < k; ++i) {
        const bool hit = last || (a.eos >= 0 && ct[i] == a.eos);
        if (hit && !last) continue;
        if (nr == 0) best_run = cs[i];
        s_par[nr] = cp[i];
        s_tok[nr] = ct[i];
        a.run_score[b * k + nr] = cs[i];
        ++nr;
      }
    }
    int nd = done;
    if (!nd) {   // HF's early-stop heuristic (can the best running beam still beat the worst finished one?) and early_stopping=True
      const int best_len = (a.early == 2 && a.lp > 0.f) ? cap : n + 1;
      const float best = best_run / (float)pow((double)best_len, (double)a.lp);
      nd = (all_fin && !(best > worst)) || (a.early == 1 && all_fin);
    }
    a.done[b] = nd;
    for (int r = 0; r < k; ++r) a.next_tok[b * k + r] = s_tok[r];
  }
  __syncthreads();
  const int64_t slot0 = (int64_t)b * k;
  // the parent is a beam of the PREVIOUS step (on the first step: beam 0 of the sample's one prefill row, which has no history yet)
  for (int idx = tid; idx < k * cap; idx += 64) {
    const int r = idx / cap, j = idx - r * cap;
    const int64_t src = (slot0 + s_par[r]) * cap + j, dst = (slot0 + r) * cap + j;
    a.anc_out[dst] = j < n ? a.anc_in[src] : (j == n ? (int)(slot0 + r) : 0);
    a.hist_out[dst] = j < n ? a.hist_in[src] : (j == n ? s_tok[r] : (int64_t)a.pad);
    const int fs = s_src[r];
    int64_t v;
    if (fs < k) {
      v = a.fin_tok_in[(slot0 + fs) * cap + j];
    } else {
      const int c = fs - k;
      v = j < n ? a.hist_in[(slot0 + cp[c]) * cap + j] : (j == n ? ct[c] : (int64_t)a.pad);
    }
    a.fin_tok_out[dst] = v;
  }
}

template <typename T>
void beam_candidates_go(const void* logits, int64_t ldl, const float* score, int B, int kin, int V, int k2, float* os, int64_t* ot, int* op,
                        hipStream_t st) {
#define GO(K2V) beam_candidates_kernel<T, K2V><<<dim3(B), dim3(CAND_NT), 0, st>>>((const T*)logits, ldl, score, kin, V, os, ot, op)
  switch (k2) {
    case 2: GO(2); break;
    case 4: GO(4); break;
    case 6: GO(6); break;
    case 8: GO(8); break;
    case 10: GO(10); break;
    case 12: GO(12); break;
    case 14: GO(14); break;
    default: GO(16); break;
  }
#undef GO
}

}  // namespace
}  // namespace mafed

using namespace mafed;

extern "C" int mafed_beam_candidates(const void* logits, mafed_dtype dtype, int64_t ldl, const float* score, int B, int kin, int V, int k,
                                     float* out_score, int64_t* out_token, int* out_parent, void* stream) {
  MAFED_CHECK_ARG(logits && score && out_score && out_token && out_parent, "beam_candidates: null pointer");
  MAFED_CHECK_ARG(B > 0 && k >= 1 && k <= 8 && kin >= 1 && kin <= k && V >= 2 * k && ldl >= V && (int64_t)kin * V < 0x7fffffffLL,
                  "beam_candidates: bad shape B=%d kin=%d k=%d V=%d ldl=%lld", B, kin, k, V, (long long)ldl);
  hipStream_t st = as_stream(stream);
  if (dtype == MAFED_F32) beam_candidates_go<float>(logits, ldl, score, B, kin, V, 2 * k, out_score, out_token, out_parent, st);
  else beam_candidates_go<bf16_t>(logits, ldl, score, B, kin, V, 2 * k, out_score, out_token, out_parent, st);
  MAFED_CHECK_LAUNCH("beam_candidates");
  return MAFED_OK;
}

extern "C" int mafed_beam_update(const float* cand_score, const int64_t* cand_token, const int* cand_parent, int B, int k, int step, int cap,
                                 int eos, int pad, int early_stopping, float length_penalty, float* run_score, const int* anc_in, int* anc_out,
                                 const int64_t* hist_in, int64_t* hist_out, const int64_t* fin_tok_in, int64_t* fin_tok_out,
                                 const float* fin_score_in, float* fin_score_out, const int* fin_len_in, int* fin_len_out, int* done,
                                 int64_t* next_token, void* stream) {
  MAFED_CHECK_ARG(cand_score && cand_token && cand_parent && run_score && anc_in && anc_out && hist_in && hist_out && fin_tok_in && fin_tok_out &&
                  fin_score_in && fin_score_out && fin_len_in && fin_len_out && done && next_token, "beam_update: null pointer");
  MAFED_CHECK_ARG(B > 0 && k >= 1 && k <= 8 && cap >= 1 && step >= 0 && step < cap && early_stopping >= 0 && early_stopping <= 2,
                  "beam_update: bad arguments B=%d k=%d step=%d cap=%d", B, k, step, cap);
  MAFED_CHECK_ARG(anc_in != anc_out && hist_in != hist_out && fin_tok_in != fin_tok_out && fin_score_in != fin_score_out && fin_len_in != fin_len_out,
                  "beam_update: the before / after buffers must be distinct");
  BeamUpdateArgs a{cand_score, cand_token, cand_parent, k, step, cap, eos, pad, early_stopping, length_penalty, run_score, anc_in, anc_out,
                   hist_in, hist_out, fin_tok_in, fin_tok_out, fin_score_in, fin_score_out, fin_len_in, fin_len_out, done, next_token};
  beam_update_kernel<<<dim3(B), dim3(64), 0, as_stream(stream)>>>(a);
  MAFED_CHECK_LAUNCH("beam_update");
  return MAFED_OK;
}
