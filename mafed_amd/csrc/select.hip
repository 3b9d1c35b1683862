// Replay-memory selection in a feature space: herding (iCaRL, Rebuffi et al. 2017) and k-center greedy (Sener &
// Savarese 2018) are the same loop around one scan, the squared distance of every row of X [n, d] to a device-resident vector v followed
// by a masked arg-best.
//
//   select_init_kernel    v := mean (fp64 and its fp32 rounding), no row taken.
//   select_scan_kernel    one pass over X, n d 4 bytes: one wave per row, score = sum_j (X[i, j] - fp32(v[j]))^2 by direct differences
//                         (k-center from its third pick on: the running minimum of the row's scores), the score stored, and the
//                         lexicographic best (score, row) of the block's eligible rows -> one partial per block.
//   select_finish_kernel  one block: folds the partials, writes picks[t] and values[t], marks the row and forms the next v
//                         (herding: r := (r + mean) - X[p] in fp64; k-center: a copy of X[p]).
// A lane's columns and the order of its sums are a function of d alone (the 16-byte path and the element-wise path read the same
// elements into the same chains), so the bits of a row's score depend on the row's contents and on v only -- duplicated rows tie
// exactly, wherever they sit -- and (score, row) pairs are totally ordered, so the folds give the same pick in any order.  The grid is
// a function of (n, d); nothing is read back by the host between picks.
#include "flat_pass.h"

namespace mafed {

constexpr int SELECT_BLOCKS_CAP = 2048;    // 8 blocks of 256 threads per CU
constexpr int SELECT_ROWS_PER_WAVE = 4;    // a block stages v once: at least this many rows per wave behind it
constexpr int SELECT_LDS_QUADS = 2048;     // v (fp32) lives in LDS up to d = 8192 (32 KB); wider rows read it through the caches
constexpr int SELECT_NONE = 0x7fffffff;    // row index of "no eligible row"

static inline int select_blocks(int64_t n) {
  const int64_t nb = cdiv(n, 4 * SELECT_ROWS_PER_WAVE);
  return (int)(nb > SELECT_BLOCKS_CAP ? SELECT_BLOCKS_CAP : nb < 1 ? 1 : nb);
}

static inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// workspace: v fp64 [d] | v fp32 [d] | scores fp32 [n] | taken int32 [n] | partial scores fp32 [cap] | partial rows int32 [cap]
struct SelectWs {
  double* v64;
  float* vf;
  float* scores;
  int* taken;
  float* pscore;
  int* prow;
  size_t bytes;
};
static inline SelectWs select_carve(void* ws, int64_t n, int64_t d) {
  SelectWs w;
  size_t o = 0;
  char* base = (char*)ws;
  w.v64 = (double*)(base + o);   o += align16((size_t)d * sizeof(double));
  w.vf = (float*)(base + o);     o += align16((size_t)d * sizeof(float));
  w.scores = (float*)(base + o); o += align16((size_t)n * sizeof(float));
  w.taken = (int*)(base + o);    o += align16((size_t)n * sizeof(int));
  w.pscore = (float*)(base + o); o += align16((size_t)SELECT_BLOCKS_CAP * sizeof(float));
  w.prow = (int*)(base + o);     o += align16((size_t)SELECT_BLOCKS_CAP * sizeof(int));
  w.bytes = o;
  return w;
}

// (score, row) a in front of b?  MINIMISE: smaller score first, else larger; equal scores: lower row.  SELECT_NONE loses to any row.
template <bool MINIMISE>
__device__ __forceinline__ bool select_better(float sa, int ia, float sb, int ib) {
  if (ia == SELECT_NONE) return false;
  if (ib == SELECT_NONE) return true;
  return (MINIMISE ? sa < sb : sa > sb) || (sa == sb && ia < ib);
}

__global__ __launch_bounds__(256) void select_init_kernel(const double* __restrict__ mean, int64_t n, int64_t d, double* __restrict__ v64,
                                                          float* __restrict__ vf, int* __restrict__ taken) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) taken[i] = 0;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < d; c += stride) {
    const double m = mean[c];
    v64[c] = m;
    vf[c] = (float)m;
  }
}

// columns 4q .. 4q + 3 of a row (VEC: one 16-byte load; otherwise element by element, zero behind column d -- the same zero the
// matching read of v gives, so such a column adds an exact 0)
template <bool VEC>
__device__ __forceinline__ float4 select_quad(const float* __restrict__ p, int64_t q, int64_t d) {
  if (VEC) return load4(p + q * 4);
  const int64_t c = q * 4;
  return make_float4(c < d ? p[c] : 0.f, c + 1 < d ? p[c + 1] : 0.f, c + 2 < d ? p[c + 2] : 0.f, c + 3 < d ? p[c + 3] : 0.f);
}

__device__ __forceinline__ void select_acc(float4& a, const float4& x, const float4& v) {
  const float ex = x.x - v.x, ey = x.y - v.y, ez = x.z - v.z, ew = x.w - v.w;
  a.x = fmaf(ex, ex, a.x);
  a.y = fmaf(ey, ey, a.y);
  a.z = fmaf(ez, ez, a.z);
  a.w = fmaf(ew, ew, a.w);
}

// grid select_blocks(n), block 256 = 4 waves, dynamic LDS: LDSV ? 16 * cdiv(d, 4) + 64 : 64 bytes.
// Lane l of a row's wave owns the quads l, l + 64, l + 128, ... of the row; component c of its quads goes into chain c in quad order,
// the four chains are added (x + y) + (z + w) and the 64 lanes by a butterfly.  FOLD_MIN: scores[i] := min(scores[i], dist), NaN sticky.
template <bool VEC, bool LDSV, bool MINIMISE, bool FOLD_MIN>
__global__ __launch_bounds__(256) void select_scan_kernel(const float* __restrict__ X, int64_t n, int64_t d, int64_t ldx,
                                                          const float* __restrict__ vf, const int* __restrict__ taken,
                                                          float* __restrict__ scores, float* __restrict__ pscore, int* __restrict__ prow) {
  extern __shared__ __attribute__((aligned(16))) float select_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nq = (d + 3) / 4;
  float* red_s = select_lds + (LDSV ? nq * 4 : 0);
  int* red_i = (int*)(red_s + 4);
  if (LDSV) {
    for (int64_t q = threadIdx.x; q < nq; q += 256) store4(select_lds + q * 4, select_quad<VEC>(vf, q, d));
    __syncthreads();
  }
  float best_s = 0.f;
  int best_i = SELECT_NONE;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n; i += nwaves) {
    const float* row = X + i * ldx;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t q = lane;
    for (; q + 192 < nq; q += 256) {   // four quads per trip: the loads of a trip are issued before the first use
      const float4 x0 = select_quad<VEC>(row, q, d), x1 = select_quad<VEC>(row, q + 64, d), x2 = select_quad<VEC>(row, q + 128, d),
                   x3 = select_quad<VEC>(row, q + 192, d);
      const float4 v0 = LDSV ? load4(select_lds + q * 4) : select_quad<VEC>(vf, q, d);
      const float4 v1 = LDSV ? load4(select_lds + (q + 64) * 4) : select_quad<VEC>(vf, q + 64, d);
      const float4 v2 = LDSV ? load4(select_lds + (q + 128) * 4) : select_quad<VEC>(vf, q + 128, d);
      const float4 v3 = LDSV ? load4(select_lds + (q + 192) * 4) : select_quad<VEC>(vf, q + 192, d);
      select_acc(a, x0, v0);
      select_acc(a, x1, v1);
      select_acc(a, x2, v2);
      select_acc(a, x3, v3);
    }
    for (; q < nq; q += 64) {
      const float4 x0 = select_quad<VEC>(row, q, d);
      const float4 v0 = LDSV ? load4(select_lds + q * 4) : select_quad<VEC>(vf, q, d);
      select_acc(a, x0, v0);
    }
    float s = wave_sum((a.x + a.y) + (a.z + a.w));
    if (FOLD_MIN) {
      const float m = scores[i];
      s = (s < m || s != s) ? s : m;
    }
    if (lane == 0) scores[i] = s;
    const bool eligible = s == s && taken[i] == 0;
    if (eligible && select_better<MINIMISE>(s, (int)i, best_s, best_i)) {
      best_s = s;
      best_i = (int)i;
    }
  }
  if (lane == 0) {
    red_s[wave] = best_s;
    red_i[wave] = best_i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (select_better<MINIMISE>(red_s[w], red_i[w], best_s, best_i)) {
        best_s = red_s[w];
        best_i = red_i[w];
      }
    pscore[blockIdx.x] = best_s;
    prow[blockIdx.x] = best_i;
  }
}

// One block.  The partials folded to the pick, then the next v.  herding: v64 := (v64 + mean) - X[p], vf its rounding; k-center: vf := X[p].
template <bool MINIMISE>
__global__ __launch_bounds__(256) void select_finish_kernel(const float* __restrict__ pscore, const int* __restrict__ prow, int nblk,
                                                            const float* __restrict__ X, int64_t d, int64_t ldx,
                                                            const double* __restrict__ mean, int herding, double* __restrict__ v64,
                                                            float* __restrict__ vf, int* __restrict__ taken, int64_t* __restrict__ pick,
                                                            float* __restrict__ value) {
  __shared__ float sm_s[256];
  __shared__ int sm_i[256];
  float bs = 0.f;
  int bi = SELECT_NONE;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    const float s = pscore[b];
    const int i = prow[b];
    if (select_better<MINIMISE>(s, i, bs, bi)) {
      bs = s;
      bi = i;
    }
  }
  sm_s[threadIdx.x] = bs;
  sm_i[threadIdx.x] = bi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w && select_better<MINIMISE>(sm_s[threadIdx.x + w], sm_i[threadIdx.x + w], sm_s[threadIdx.x], sm_i[threadIdx.x])) {
      sm_s[threadIdx.x] = sm_s[threadIdx.x + w];
      sm_i[threadIdx.x] = sm_i[threadIdx.x + w];
    }
    __syncthreads();
  }
  const int p = sm_i[0];
  if (p == SELECT_NONE) {   // no eligible row is left: v stays, every later pick ends here too
    if (threadIdx.x == 0) {
      *pick = -1;
      *value = __builtin_nanf("");
    }
    return;
  }
  if (threadIdx.x == 0) {
    *pick = p;
    *value = sm_s[0];
    taken[p] = 1;
  }
  const float* row = X + (int64_t)p * ldx;
  for (int64_t c = threadIdx.x; c < d; c += 256) {
    const float x = row[c];
    if (herding) {
      const double r = (v64[c] + mean[c]) - (double)x;
      v64[c] = r;
      vf[c] = (float)r;
    } else {
      vf[c] = x;
    }
  }
}

template <bool VEC, bool LDSV>
static void select_scan_launch(bool minimise, bool fold_min, int nblk, size_t lds, hipStream_t st, const float* X, int64_t n, int64_t d,
                               int64_t ldx, const SelectWs& w, float* scores) {
  const double bytes = 4.0 * (double)n * (double)d;
  const dim3 grid((unsigned)nblk), block(256);
  if (minimise)
    launch(K_SMALL, bytes, select_scan_kernel<VEC, LDSV, true, false>, grid, block, lds, st, X, n, d, ldx, (const float*)w.vf,
           (const int*)w.taken, scores, w.pscore, w.prow);
  else if (!fold_min)
    launch(K_SMALL, bytes, select_scan_kernel<VEC, LDSV, false, false>, grid, block, lds, st, X, n, d, ldx, (const float*)w.vf,
           (const int*)w.taken, scores, w.pscore, w.prow);
  else
    launch(K_SMALL, bytes, select_scan_kernel<VEC, LDSV, false, true>, grid, block, lds, st, X, n, d, ldx, (const float*)w.vf,
           (const int*)w.taken, scores, w.pscore, w.prow);
}

}  // namespace mafed

using namespace mafed;

extern "C" size_t mafed_select_workspace_bytes(int64_t n, int64_t d) {
  if (n < 0 || d < 0) return 0;
  return select_carve(nullptr, n, d).bytes;
}

extern "C" int mafed_select_greedy(const float* X, int64_t n, int64_t d, int64_t ldx, const double* mean, int mode, int64_t k, int64_t* picks,
                                   float* values, float* last_scores, void* workspace, size_t workspace_bytes, void* stream) {
  MAFED_CHECK_ARG(X && mean && picks && values && n >= 1 && n < SELECT_NONE && d >= 1 && ldx >= d && k >= 1 && k <= n &&
                      (mode == MAFED_SELECT_HERDING || mode == MAFED_SELECT_KCENTER),
                  "select_greedy: bad arguments (n=%lld d=%lld ldx=%lld k=%lld mode=%d)", (long long)n, (long long)d, (long long)ldx,
                  (long long)k, mode);
  const size_t need = mafed_select_workspace_bytes(n, d);
  if (!workspace || workspace_bytes < need) {
    set_error("select_greedy: workspace %zu < %zu", workspace_bytes, need);
    return MAFED_EWORKSPACE;
  }
  MAFED_CHECK_ARG(aligned16({workspace}), "select_greedy: the workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const SelectWs w = select_carve(workspace, n, d);
  float* scores = last_scores ? last_scores : w.scores;
  const bool herding = mode == MAFED_SELECT_HERDING;
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && aligned16({X});
  const int64_t nq = (d + 3) / 4;
  const bool ldsv = nq <= SELECT_LDS_QUADS;
  const size_t lds = (ldsv ? (size_t)nq * 16 : 0) + 64;
  const int nblk = select_blocks(n);
  const int64_t init_elems = n > d ? n : d;
  launch(K_SMALL, 4.0 * n + 20.0 * d, select_init_kernel, dim3((unsigned)(cdiv(init_elems, 256) > 1024 ? 1024 : cdiv(init_elems, 256))),
         dim3(256), 0, st, mean, n, d, w.v64, w.vf, w.taken);
  MAFED_CHECK_LAUNCH("select_greedy(init)");
  for (int64_t t = 0; t < k; ++t) {
    const bool minimise = herding || t == 0, fold_min = !herding && t >= 2;
    if (vec && ldsv) select_scan_launch<true, true>(minimise, fold_min, nblk, lds, st, X, n, d, ldx, w, scores);
    else if (vec) select_scan_launch<true, false>(minimise, fold_min, nblk, lds, st, X, n, d, ldx, w, scores);
    else if (ldsv) select_scan_launch<false, true>(minimise, fold_min, nblk, lds, st, X, n, d, ldx, w, scores);
    else select_scan_launch<false, false>(minimise, fold_min, nblk, lds, st, X, n, d, ldx, w, scores);
    MAFED_CHECK_LAUNCH("select_greedy(scan)");
    if (minimise)
      launch(K_SMALL, 8.0 * nblk + 20.0 * d, select_finish_kernel<true>, dim3(1), dim3(256), 0, st, (const float*)w.pscore, (const int*)w.prow,
             nblk, X, d, ldx, mean, (int)herding, w.v64, w.vf, w.taken, picks + t, values + t);
    else
      launch(K_SMALL, 8.0 * nblk + 20.0 * d, select_finish_kernel<false>, dim3(1), dim3(256), 0, st, (const float*)w.pscore, (const int*)w.prow,
             nblk, X, d, ldx, mean, (int)herding, w.v64, w.vf, w.taken, picks + t, values + t);
    MAFED_CHECK_LAUNCH("select_greedy(finish)");
  }
  return MAFED_OK;
}
