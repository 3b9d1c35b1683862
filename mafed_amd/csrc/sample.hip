// Sampled decoding (model.sample): one launch turns R rows of V logits into R drawn tokens.  It replaces what transformers'
// GenerationMixin._sample runs per token -- TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, MinPLogitsWarper, softmax and
// torch.multinomial -- and the eos / pad tail of the greedy pick.
//
// One 1024-thread workgroup per row; the row is read once and stays in registers (z = logit / temperature; wave w owns the ids
// [w * IT * 64, (w + 1) * IT * 64), register j of lane l holding id w * IT * 64 + j * 64 + l, so every load is 64 consecutive elements).
//
//   kept set   {z >= max(z_k, z*) and z - z_max >= log(min_p)}: z_k the k-th largest z (ties kept), z* the largest value with
//              mass{z > z*} < top_p * mass(top-k survivors) <= mass{z >= z*} (ties on the cut are all kept: the one deviation from
//              TopPLogitsWarper, which keeps an order-dependent part of such a tie).  Both thresholds come from the same radix descent over
//              the order-preserving 32-bit image of z: four passes of 8-bit digits, an LDS histogram per pass of counts (top-k) or
//              masses (top-p) restricted to the digits chosen so far.
//   mass       floor(exp(z - z_max) * 2^47) as a 64-bit integer (V <= 65 536, so a row's sum stays below 2^63).  Integer sums do not
//              depend on their order: the histograms take plain LDS atomics, the cumulative sum needs no fixed tree, and a row's result
//              is the same bits on every run whatever R is.  Dropping what lies below 2^-47 of the top token moves the CDF by < 2^-31.
//   draw       u from Philox4x32-10 (key = the halves of *seed, counter = (row, step, 0, 0), u = ((x0 >> 8) + 0.5) * 2^-24 in fp32) or from
//              `uniforms`; the token is the first kept id, ascending, whose inclusive cumulative mass exceeds floor(u * Z).  Found in two
//              levels: the wave whose id range holds the crossing (16 wave totals), then that wave's masses, laid out in id order in LDS.
//
// No global atomics, no workspace; the registers are recomputed into masses where needed (v_exp_f32) instead of being held twice.
// At 1024 threads the row plus the loops' temporaries fill the 128 VGPRs a thread may have: the compiler spills about twenty values to
// scratch, all between the phases and none inside a loop over the row (DESIGN.md section 4c'' has the figures).
// Measured on an MI355X at V = 50 304 (profiles/sample_decode.txt): 24 us without warpers, 64 us with top-k and top-p (about 5 us per
// radix pass), flat from 32 to 160 rows.
#include "common.h"

namespace mafed {
namespace {

typedef unsigned long long u64;

constexpr int SAMPLE_NT = 1024, SAMPLE_NW = SAMPLE_NT / 64;
constexpr uint32_t KEY_FLOOR = 0x00800000u;   // ord_f32(-inf) + 1: every finite value and nothing else (a negative NaN sits below)
constexpr float MASS_ONE = 140737488355328.f;   // 2^47

__device__ __forceinline__ uint32_t ord_f32(float v) {   // order-preserving image of an fp32 value (as in beam.hip)
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_down_u64(u64 v, int o) {
  const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up_u64(u64 v, int o) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}

// The row's registers are re-read through this in every loop over them: it keeps the compiler from carrying a second copy of the row
// (the keys, or the masses of an earlier loop) in registers across the loops, which would spill.
__device__ __forceinline__ float reread(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// floor(exp(z - zmax) * 2^47), z <= zmax.  exp through v_exp_f32 on (z - zmax) * log2(e), the product carried with log2(e)'s low part.
__device__ __forceinline__ u64 mass_of(float z, float zmax) {
  const float d = z - zmax;
  const float y = fmaf(d, 1.92596303e-8f, d * 1.44269502f);
  // (d is NaN for a NaN logit, or in a row without a finite value, where z_max = -inf: such an element has no mass -- the integer
  //  conversion never sees a NaN.  A NaN logit still orders above every number in ord_f32, so it can take a top-k / top-p slot; it
  //  cannot be drawn.)
  return d <= 0.f ? (u64)(__builtin_amdgcn_exp2f(y) * MASS_ONE) : 0ull;
}

// Philox4x32-10 (Salmon et al., SC'11; Random123): -> the first output word
__device__ __forceinline__ uint32_t philox4x32_10_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

struct SampleArgs {
  const void* logits;
  int64_t ldl;
  int V;
  float temperature;
  int top_k;
  float top_p, min_p;
  const uint64_t* seed;
  int step;
  const float* uniforms;
  int64_t* unfinished;
  int eos, pad;
  int64_t* token;
  float* logprob;
  int* kept;
};

// The largest key K among the elements with key >= kmin such that W{key > K} < target <= W{key >= K}; W counts (MASS = false: K is
// the target-th largest) or adds masses (MASS = true: target = ceil(frac * W{key >= kmin}), taken from the first pass's histogram).
// A thread adds runs of equal digits as one atomic, so a row whose values share their leading digits does not serialise on one bin.
template <int IT, bool MASS>
__device__ uint32_t radix_select(const float (&z)[IT], float zmax, uint32_t kmin, u64 target, float frac, u64* s_hist, u64* s_bc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t prefix = 0u, mask = 0u;
  u64 above = 0ull;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) s_hist[tid] = 0ull;
    __syncthreads();
    int cur = -1;
    u64 acc = 0ull;
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const float zj = reread(z[j]);
      const uint32_t key = ord_f32(zj);
      if (key >= kmin && ((key ^ prefix) & mask) == 0u) {
        const int d = (int)((key >> shift) & 255u);
        if (d != cur) {
          if (acc) atomicAdd(&s_hist[cur], acc);
          cur = d;
          acc = 0ull;
        }
        acc += MASS ? mass_of(zj, zmax) : 1ull;
      }
    }
    if (acc) atomicAdd(&s_hist[cur], acc);
    __syncthreads();
    if (wave == 0) {   // suffix sums over the 256 bins (lane l: bins 4l .. 4l+3), then the highest digit whose suffix reaches the target
      const u64 h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
      u64 suf = h0 + h1 + h2 + h3;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 v = shfl_down_u64(suf, o);
        if (lane + o < 64) suf += v;
      }
      if (MASS && shift == 24) {
        const u64 total = shfl_u64(suf, 0);
        const double pd = (double)frac * (double)total;
        target = (u64)pd;
        if ((double)target < pd) ++target;
        target = target < 1ull ? 1ull : (target > total ? total : target);
      }
      const u64 ballot = __ballot(above + suf >= target);
      const int L = ballot ? 63 - __clzll((long long)ballot) : 0;
      if (lane == L) {
        const u64 rest = suf - (h0 + h1 + h2 + h3), S3 = rest + h3, S2 = S3 + h2, S1 = S2 + h1;
        int d;
        u64 inc;
        if (above + S3 >= target) { d = 3; inc = rest; }
        else if (above + S2 >= target) { d = 2; inc = S3; }
        else if (above + S1 >= target) { d = 1; inc = S2; }
        else { d = 0; inc = S1; }
        s_bc[0] = (u64)(4 * L + d);
        s_bc[1] = inc;
        s_bc[2] = target;
      }
    }
    __syncthreads();
    prefix |= (uint32_t)s_bc[0] << shift;
    mask |= 255u << shift;
    above += s_bc[1];
    target = s_bc[2];
  }
  return prefix;
}

template <typename T, int IT>
__global__ __launch_bounds__(SAMPLE_NT) void sample_token_kernel(SampleArgs a) {
  __shared__ u64 s_hist[256];
  __shared__ u64 s_bc[4];
  __shared__ u64 s_wq[SAMPLE_NW];
  __shared__ int s_wc[SAMPLE_NW];
  __shared__ float s_red[SAMPLE_NW];
  __shared__ u64 s_q[IT * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x, V = a.V;
  if (a.unfinished && a.unfinished[row] == 0) {   // a finished row emits pad (the whole workgroup leaves: the flag is per row)
    if (tid == 0) {
      a.token[row] = (int64_t)a.pad;
      if (a.logprob) a.logprob[row] = 0.f;
      if (a.kept) a.kept[row] = 0;
    }
    return;
  }
  const T* lg = reinterpret_cast<const T*>(a.logits) + (int64_t)row * a.ldl;
  const int id0 = wave * IT * 64 + lane;
  float z[IT];
  float lmax = -INFINITY;
#pragma unroll
  for (int j = 0; j < IT; ++j) {
    const int i = id0 + j * 64;
    const float l = i < V ? Elem<T>::load(lg + i) : -INFINITY;
    lmax = fmaxf(lmax, l);
    z[j] = reread(l / a.temperature);   // (also ends the quotient's temporaries here: the loads are batched, the divisions are not)
  }
  lmax = block_max<SAMPLE_NT>(lmax, s_red);
  const float zmax = lmax / a.temperature;   // the same division as every element's: the maximum of z, bit for bit
  uint32_t kthr = KEY_FLOOR;
  if (a.top_k > 0 && a.top_k < V) {
    const uint32_t k = radix_select<IT, false>(z, zmax, KEY_FLOOR, (u64)a.top_k, 0.f, s_hist, s_bc);
    kthr = k > kthr ? k : kthr;
  }
  if (a.top_p < 1.f) {
    const uint32_t k = radix_select<IT, true>(z, zmax, kthr, 0ull, a.top_p, s_hist, s_bc);
    kthr = k > kthr ? k : kthr;
  }
  const float lmin = a.min_p > 0.f ? logf(a.min_p) : -INFINITY;
  // kept masses: per thread, per wave, then over the waves in id order
  u64 tq = 0ull;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < IT; ++j) {
    const float zj = reread(z[j]);
    if (ord_f32(zj) >= kthr && zj - zmax >= lmin) {
      ++cnt;
      tq += mass_of(zj, zmax);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    tq += shfl_xor_u64(tq, o);
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane == 0) { s_wq[wave] = tq; s_wc[wave] = cnt; }
  __syncthreads();
  u64 Z = 0ull;
  int nkept = 0;
#pragma unroll
  for (int w = 0; w < SAMPLE_NW; ++w) { Z += s_wq[w]; nkept += s_wc[w]; }
  float u;
  if (a.uniforms) {
    u = a.uniforms[row];
  } else {
    const uint64_t seed = *a.seed;
    u = ((float)(philox4x32_10_x0((uint32_t)row, (uint32_t)a.step, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32)) >> 8) + 0.5f) * 5.9604644775390625e-8f;
  }
  u64 t = (u64)((double)u * (double)Z);   // cum > u * Z  <=>  cum > floor(u * Z) for an integer cum
  if (Z > 0ull && t >= Z) t = Z - 1ull;
  int wsel = -1;
  u64 base = 0ull, cum = 0ull;
#pragma unroll
  for (int w = 0; w < SAMPLE_NW; ++w) {
    const u64 nxt = cum + s_wq[w];
    if (wsel < 0 && nxt > t) { wsel = w; base = cum; }
    cum = nxt;
  }
  if (wsel < 0) {   // no finite logit in the row (Z = 0): nothing can be drawn
    if (tid == 0) {
      a.token[row] = (int64_t)a.pad;
      if (a.logprob) a.logprob[row] = -INFINITY;
      if (a.kept) a.kept[row] = 0;
    }
    return;
  }
  if (wave == wsel) {
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const float zj = reread(z[j]);
      s_q[j * 64 + lane] = (ord_f32(zj) >= kthr && zj - zmax >= lmin) ? mass_of(zj, zmax) : 0ull;
    }
  }
  __syncthreads();
  if (wave != wsel) return;
  u64 own = 0ull;
  for (int jj = 0; jj < IT; ++jj) own += s_q[lane * IT + jj];   // lane l: ids l * IT .. l * IT + IT - 1 of the wave's range
  u64 incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 v = shfl_up_u64(incl, o);
    if (lane >= o) incl += v;
  }
  const u64 ballot = __ballot(base + incl > t);   // not empty: base + the wave's total > t
  const int L = __ffsll((long long)ballot) - 1;
  if (lane != L) return;
  u64 c = base + incl - own;
  int jj = 0;
  for (; jj < IT - 1; ++jj) {
    c += s_q[lane * IT + jj];
    if (c > t) break;
  }
  const int tok = wsel * IT * 64 + lane * IT + jj;
  a.token[row] = (int64_t)tok;
  if (a.kept) a.kept[row] = nkept;
  if (a.logprob) {
    const double zt = ((double)Elem<T>::load(lg + tok) - (double)lmax) / (double)a.temperature;
    a.logprob[row] = (float)(zt - (log((double)Z) - 47.0 * 0.69314718055994530942));
  }
  if (a.unfinished && a.eos >= 0 && tok == a.eos) a.unfinished[row] = 0;
}

template <typename T>
void sample_token_go(const SampleArgs& a, int R, hipStream_t st) {
  const dim3 grid(R), block(SAMPLE_NT);
  if (a.V <= 1 * SAMPLE_NT) sample_token_kernel<T, 1><<<grid, block, 0, st>>>(a);
  else if (a.V <= 8 * SAMPLE_NT) sample_token_kernel<T, 8><<<grid, block, 0, st>>>(a);
  else if (a.V <= 50 * SAMPLE_NT) sample_token_kernel<T, 50><<<grid, block, 0, st>>>(a);
  else sample_token_kernel<T, 64><<<grid, block, 0, st>>>(a);
}

}  // namespace
}  // namespace mafed

using namespace mafed;

extern "C" int mafed_sample_token(const void* logits, mafed_dtype dtype, int64_t ldl, int R, int V, float temperature, int top_k, float top_p,
                                  float min_p, const uint64_t* seed, int step, const float* uniforms, int64_t* unfinished, int eos, int pad,
                                  int64_t* token, float* logprob, int* kept, void* stream) {
  MAFED_CHECK_ARG(logits && token && (seed || uniforms), "sample_token: null pointer (logits, token, and one of seed / uniforms)");
  MAFED_CHECK_ARG(dtype == MAFED_F32 || dtype == MAFED_BF16, "sample_token: dtype must be fp32 or bf16");
  MAFED_CHECK_ARG(R >= 1 && V >= 1 && V <= 64 * SAMPLE_NT && ldl >= V && step >= 0, "sample_token: bad shape R=%d V=%d (<= 65536) ldl=%lld step=%d",
                  R, V, (long long)ldl, step);
  MAFED_CHECK_ARG(temperature > 0.f && top_k >= 0 && top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p < 1.f,
                  "sample_token: temperature %g (> 0), top_k %d (>= 0), top_p %g (0, 1], min_p %g [0, 1)", (double)temperature, top_k, (double)top_p,
                  (double)min_p);
  const SampleArgs a{logits, ldl, V, temperature, top_k, top_p, min_p, seed, step, uniforms, unfinished, eos, pad, token, logprob, kept};
  if (dtype == MAFED_F32) sample_token_go<float>(a, R, as_stream(stream));
  else sample_token_go<bf16_t>(a, R, as_stream(stream));
  MAFED_CHECK_LAUNCH("sample_token");
  return MAFED_OK;
}
