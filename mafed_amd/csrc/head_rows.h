// The one copy of what the fused head losses share (CE: ce.hip; CE + KL: kd.hip; CE + MSE against stored logits: der.hip; squared norm:
// sqnorm.hip; token log-probability: score.hip).
// All are one-256-thread-block-per-row passes over a [B * Tn, V] logits matrix: the row -> (b, t) map with its shifted label, the
// per-sample normaliser, the zero store of an unlabelled row's gradient, the float4 online log-sum-exp of a row, the one-block finalize
// kernel and the entry points' refusals and launch dispatch.  A kernel's body shows its arithmetic and nothing else; a new head loss is
// a row body for each direction, its entry points and a line in engine.py's _head_text.
#pragma once
#include "common.h"

namespace mafed {

// Row r = blockIdx.x of the head is text position t of sample b and predicts labels[b, t + 1] (logits[..., :-1, :] against
// labels[..., 1:], mafed/model/vl_pythia.py:91): the last position predicts nothing, -100 is the ignore index.  Everything is
// block-uniform.  The label is loaded where a kernel asks for it, not here: the CE forward wants it in one thread, after the row.
struct HeadRow {
  const int64_t* labels;
  int Tn;
  int64_t r, r0;   // r0 = b Tn: the sample's first row, and its first label
  int b, t;
  __device__ __forceinline__ HeadRow(const int64_t* labels_, int Tn_)
      : labels(labels_), Tn(Tn_), r(blockIdx.x), r0((int64_t)(int)(r / Tn_) * Tn_), b((int)(r / Tn_)), t((int)(r - r0)) {}
  __device__ __forceinline__ bool last() const { return t == Tn - 1; }
  __device__ __forceinline__ int64_t next_label() const { return labels[r0 + t + 1]; }   // (of a row that is not the last)
  __device__ __forceinline__ int64_t label() const { return t < Tn - 1 ? next_label() : -100; }
  __device__ __forceinline__ bool labelled() const { return label() != -100; }
  // B max(count_b, 1e-13), count_b = the labelled rows of sample b: what a row's gradient scale is divided by.  A kernel keeps its own
  // division -- (2 dloss) / den and 2 (dloss / den) are different bits.
  __device__ __forceinline__ float denominator(int B) const {
    float cnt = 0.f;
    for (int tt = 1; tt < Tn; ++tt) cnt += (labels[r0 + tt] != -100) ? 1.f : 0.f;
    return (float)B * fmaxf(cnt, 1e-13f);
  }
  // the rank of this row among its sample's labelled rows (0 for the first one): the labelled rows in front of it.  The same number on
  // the dense head and on the row-sparse head's compact labels, which list a sample's labelled rows in ascending t (der.hip).
  __device__ __forceinline__ int rank() const {
    int j = 0;
    for (int tt = 1; tt <= t; ++tt) j += (labels[r0 + tt] != -100) ? 1 : 0;
    return j;
  }
};

// zeros over dx[0 .. V): an unlabelled row's gradient, in the kernel's own vectors of VEC elements (8 or 16 bytes; +0 is all-zero bits)
template <typename T, int VEC = 4>
__device__ __forceinline__ void zero_row(T* dx, int64_t V) {
  static_assert(VEC * sizeof(T) == 8 || VEC * sizeof(T) == 16, "8- or 16-byte stores");
  for (int64_t c = (int64_t)threadIdx.x * VEC; c < V; c += 256 * VEC) {
    if constexpr (VEC * sizeof(T) == 16) *reinterpret_cast<uint4*>(dx + c) = make_uint4(0u, 0u, 0u, 0u);
    else *reinterpret_cast<uint2*>(dx + c) = make_uint2(0u, 0u);
  }
}

// log-sum-exp of a row as the block holds it: lse = gm + log(gs), gs = sum exp(x - gm); value() where it is wanted (one thread)
struct RowLse {
  float gm, gs;
  __device__ __forceinline__ float value() const { return gm + logf(gs); }
};

// block combine of the threads' online (max, sum) pairs; sm holds 8 floats.  (A thread that saw no column keeps its empty sum out.)
__device__ __forceinline__ RowLse block_lse(float m, float s, float* sm) {
  const float gm = block_max<256>(m, sm);
  s = (m == -INFINITY) ? 0.f : s * expf(m - gm);
  return {gm, block_sum<256>(s, sm)};
}

// online log-sum-exp of x[0 .. V) with 4-element vector loads (V % 4 == 0, x on a 4-element boundary): each thread walks its columns in
// ascending order, the block combines in one fixed tree.  expf / logf: kd.hip's accumulators (__expf, contraction off) are another thing.
template <typename T>
__device__ __forceinline__ RowLse row_lse4(const T* x, int64_t V, float* sm) {
  float m = -INFINITY, s = 0.f;
  for (int64_t c = (int64_t)threadIdx.x * 4; c < V; c += 256 * 4) {
    const float4 v = load4(x + c);
    const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (mx > m) { s *= expf(m - mx); m = mx; }
    s += (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m));
  }
  return block_lse(m, s, sm);
}

// One trip of row_lse4's loop, for a kernel that walks a second matrix beside x in the same loop (der.hip): the statements above, word
// for word, so that (m, s) -- and block_lse of them -- are row_lse4's bits.  row_lse4 keeps its own loop: routed through this function
// the compiler schedules the cross-entropy forward differently.
__device__ __forceinline__ void lse4_step(float& m, float& s, const float4 v) {
  const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
  if (mx > m) { s *= expf(m - mx); m = mx; }
  s += (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m));
}

// mean_b( sum_t rows[k][b, t] / max(count_b, 1e-13) ) over the labelled rows, for the N row arrays of a forward, each summed on its
// own: one wave per sample, lanes over t, the four waves folded in fixed order; a single block.  N = 1 (CE, squared norm): out[0].
// N = 2: out[0 .. 3) = {w0 v0 + coef v1, v0, v1} (CE + KL: w0 = 1, which leaves v0's bits alone; CE + MSE: beta, alpha).  `poison` (may
// be null): a device flag; non-zero turns out[0], and only it, into NaN (mafed_ce_fwd_guarded: the row-sparse head's overflow flag).
template <int N>
__global__ __launch_bounds__(256) void head_finalize_kernel(const float* __restrict__ rows0, const float* __restrict__ rows1,
                                                            const int64_t* __restrict__ labels, int B, int Tn, float w0, float coef,
                                                            float* __restrict__ out, const int* __restrict__ poison) {
  static_assert(N == 1 || N == 2, "one or two row arrays");
  __shared__ float sm[4 * N];
  const float* rows[2] = {rows0, rows1};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[N] = {};
  for (int b = wave; b < B; b += 4) {
    float s[N] = {}, c = 0.f;
    for (int t = lane; t < Tn - 1; t += 64) {
      if (labels[(int64_t)b * Tn + t + 1] != -100) {
        c += 1.f;
        for (int k = 0; k < N; ++k) s[k] += rows[k][(int64_t)b * Tn + t];
      }
    }
    c = wave_sum(c);
    for (int k = 0; k < N; ++k) acc[k] += wave_sum(s[k]) / fmaxf(c, 1e-13f);
  }
  if (lane == 0)
    for (int k = 0; k < N; ++k) sm[4 * k + wave] = acc[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    float v[N];
    for (int k = 0; k < N; ++k) v[k] = ((sm[4 * k] + sm[4 * k + 1]) + (sm[4 * k + 2] + sm[4 * k + 3])) / (float)B;
    float first = v[0];
    if constexpr (N == 2) {
      first = fmaf(coef, v[1], __fmul_rn(w0, v[0]));   // (w0 == 1: the one fma that v0 + coef v1 has always compiled to)
      out[1] = v[0];
      out[2] = v[1];
    }
    out[0] = (poison && poison[0] != 0) ? __int_as_float(0x7fc00000) : first;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// What every head entry point refuses first, with the texts callers see (who = the entry point's name without the prefix)
#define MAFED_HEAD_CHECK_PTRS(ok, who) MAFED_CHECK_ARG(ok, "%s: null pointer", who)
#define MAFED_HEAD_CHECK_SHAPE(B, T, V, who) \
  MAFED_CHECK_ARG((B) > 0 && (T) > 0 && (V) > 0 && (V) % 4 == 0, "%s: bad shape (V must be a multiple of 4)", who)

// The launch shape of a pass over the head rows: a 256-thread block per row, `bytes` = one [B * T, V] matrix of the dtype (the
// profiler's work unit: a kernel moves a whole number of them)
struct HeadPass {
  mafed_dtype dtype;
  hipStream_t st;
  dim3 grid, block;
  double bytes;
  HeadPass(mafed_dtype dtype_, int B, int T, int64_t V, void* stream)
      : dtype(dtype_), st(as_stream(stream)), grid((unsigned)((int64_t)B * T)), block(256),
        bytes((double)B * T * V * (dtype_ == MAFED_F32 ? 4.0 : 2.0)) {}

  // kernel<float> or kernel<bf16_t> by the dtype: pick(T{}) returns the instantiation; launch() casts the entry point's void pointers
  // to the kernel's parameter types
  template <class Pick, typename... Args>
  void rows(int tag, double matrices, Pick pick, Args... args) const {
    if (dtype == MAFED_F32) launch(tag, matrices * bytes, pick(float{}), grid, block, 0, st, args...);
    else launch(tag, matrices * bytes, pick(bf16_t{}), grid, block, 0, st, args...);
  }

  // the finalize kernel behind a forward (tag K_SMALL, no bytes worth counting)
  template <int N>
  void finalize(const float* rows0, const float* rows1, const int64_t* labels, int B, int T, float coef, float* out, const int* poison,
                float w0 = 1.0f) const {
    launch(K_SMALL, 0.0, head_finalize_kernel<N>, dim3(1), block, 0, st, rows0, rows1, labels, B, T, w0, coef, out, poison);
  }
};

}  // namespace mafed
