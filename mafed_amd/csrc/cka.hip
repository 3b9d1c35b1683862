// Representation-drift analysis (mafed/analysis/get_average_CKA_per_layer.py, mafed/analysis/cka.py): per-sample modality pooling
// of the hidden states and the centred cross-Gram Frobenius norm ||(X - 1 mu_x^T)^T (Y - 1 mu_y^T)||_F^2 behind linear CKA.
//
//   cka_pool_kernel    one block per (sample, layer, modality): the fp64 mean of the image rows [0, P) or the last txt_len rows of the
//                      sample's hidden state, txt_len = sum of its text attention mask (a literal port of :109-117).
//   cka_colsum_kernel  fp64 column-sum partials of G feature sets over 1024-row chunks; cka_mean_kernel sums them in chunk order.
//   cka_rownorm_kernel ||x_r - mu||^2 per row in fp64 (the debiased estimator's sum_squared_rows, cka.py:144-147).
//   cka_hsic_kernel    one 128 x 128 tile of C = Xc^T Yc per block on v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chains), the operands
//                      centred in fp64 on their way into LDS (never Xt Y - n mu_x mu_y^T: Pythia's residual stream has a few huge
//                      dimensions and that form cancels).  C never leaves the registers: every HSIC_CHUNK rows the MFMA accumulators
//                      are flushed into a second set of fp32 accumulators, so an element of C goes through at most HSIC_CHUNK fmaf
//                      roundings plus n / HSIC_CHUNK adds instead of n (fp64 second-level accumulators cost 128 more VGPRs, one wave
//                      per SIMD instead of two: 68 instead of 95 TF measured), and the epilogue writes the tile's fp64 sum of
//                      squares.  Self terms (X is Y) run only the tiles i <= j and count the off-diagonal ones twice.
//   cka_hsic_finish    sums each product's tile partials in a fixed tree.
// Every reduction has a fixed order and every product is computed by the same blocks whatever else is in the batch, so the results are
// bitwise reproducible across runs and batch compositions.
#include "common.h"

namespace mafed {

constexpr int POOL_MAX_LAYERS = 64;
struct PoolLayers {
  const float* p[POOL_MAX_LAYERS];
};

// grid (B, L, 2), block 256; out [2, L, n, h]
__global__ __launch_bounds__(256) void cka_pool_kernel(PoolLayers layers, int S, int P, int h, const int64_t* __restrict__ mask, int T,
                                                       const int64_t* __restrict__ rows, int64_t n, float* __restrict__ out) {
  const int b = blockIdx.x, l = blockIdx.y, mod = blockIdx.z, L = gridDim.y;
  int r0, cnt;
  if (mod == 0) {
    r0 = 0;
    cnt = P;
  } else {
    int64_t s = 0;
    for (int t = 0; t < T; ++t) s += mask[(int64_t)b * T + t];   // every thread, same order: no reduction needed for T <= a few hundred
    cnt = (int)(s < 0 ? 0 : (s > S ? S : s));   // (a 0/1 mask never clamps; anything else must not read outside the sample)
    r0 = S - cnt;
  }
  const float* src = layers.p[l] + (int64_t)b * S * h;
  const int64_t row = rows ? rows[b] : b;
  if (row < 0 || row >= n) return;   // (documented: such a sample is dropped)
  float* dst = out + (((int64_t)mod * L + l) * n + row) * h;
  const double inv = 1.0 / (double)cnt;   // cnt == 0: 0 * inf -> NaN, as numpy's mean of an empty slice
  for (int c = threadIdx.x; c < h; c += 256) {
    double a0 = 0.0, a1 = 0.0;
    int r = 0;
    for (; r + 1 < cnt; r += 2) {
      a0 += (double)src[(int64_t)(r0 + r) * h + c];
      a1 += (double)src[(int64_t)(r0 + r + 1) * h + c];
    }
    if (r < cnt) a0 += (double)src[(int64_t)(r0 + r) * h + c];
    dst[c] = (float)((a0 + a1) * inv);
  }
}

constexpr int STAT_ROWS = 1024;   // rows per column-sum partial

// grid (cdiv(h, 64), cdiv(n, STAT_ROWS), G), block 256 = 64 columns x 4 row lanes; partial [G, chunks, h]
__global__ __launch_bounds__(256) void cka_colsum_kernel(const float* __restrict__ X, int64_t n, int64_t h, int64_t ldx, int64_t set_stride,
                                                         double* __restrict__ partial) {
  __shared__ double sm[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cx, g = blockIdx.z;
  const int64_t r0 = (int64_t)blockIdx.y * STAT_ROWS, r1 = min(n, r0 + STAT_ROWS);
  const float* x = X + g * set_stride;
  double a = 0.0;
  if (c < h)
    for (int64_t r = r0 + ry; r < r1; r += 4) a += (double)x[r * ldx + c];
  sm[ry][cx] = a;
  __syncthreads();
  if (ry == 0 && c < h) partial[(g * gridDim.y + blockIdx.y) * h + c] = ((sm[0][cx] + sm[1][cx]) + (sm[2][cx] + sm[3][cx]));
}

// grid (cdiv(h, 256), G)
__global__ __launch_bounds__(256) void cka_mean_kernel(const double* __restrict__ partial, int chunks, int64_t n, int64_t h,
                                                       double* __restrict__ mean) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
  if (c >= h) return;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += partial[(g * chunks + k) * h + c];
  mean[g * h + c] = s / (double)n;
}

// grid (cdiv(n, 4), G), block 256: one wave per row
__global__ __launch_bounds__(256) void cka_rownorm_kernel(const float* __restrict__ X, int64_t n, int64_t h, int64_t ldx, int64_t set_stride,
                                                          const double* __restrict__ mean, double* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), g = blockIdx.y;
  const int lane = threadIdx.x & 63;
  if (r >= n) return;
  const float* x = X + g * set_stride + r * ldx;
  const double* mu = mean + g * h;
  double a = 0.0;
  for (int64_t c = lane; c < h; c += 64) {
    const double d = (double)x[c] - mu[c];
    a += d * d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0) out[g * n + r] = a;
}

// ---- HSIC ----------------------------------------------------------------------------------------------------------------------------------
constexpr int HT = 128;            // output tile edge
constexpr int HBK = 16;            // rows of X / Y per LDS stage
constexpr int HLD = HT + 32;       // LDS row stride: the two half-waves of an operand read hit disjoint banks
constexpr int HSIC_CHUNK = 4096;   // rows between flushes of the MFMA accumulators into the second-level ones
constexpr int HSIC_MAX_BATCH = 24; // products per launch (descriptors travel in the kernel arguments)

struct HsicProd {
  const float* x;
  const float* y;
  const double* mx;
  const double* my;
  int64_t ldx, ldy;
  int n, hx, hy, sym;
};
struct HsicBatch {
  int count;
  int tile_start[HSIC_MAX_BATCH + 1];   // prefix sums of the products' tile counts
  HsicProd p[HSIC_MAX_BATCH];
};

__host__ __device__ inline int hsic_tiles(int hx, int hy, int sym) {
  const int tx = (hx + HT - 1) / HT, ty = (hy + HT - 1) / HT;
  return sym ? tx * (tx + 1) / 2 : tx * ty;
}

typedef __attribute__((ext_vector_type(16))) float f32x16;

// raw rows [k0, k0 + HBK) of one operand column into registers (the loads stay in flight across the current stage's MFMAs) ...
__device__ __forceinline__ void hsic_fetch(const float* __restrict__ src, int64_t ld, int n, int col, bool col_ok, int k0, int rsub,
                                           float (&v)[HBK / 2]) {
#pragma unroll
  for (int i = 0; i < HBK / 2; ++i) {
    const int r = k0 + rsub + 2 * i;
    v[i] = (col_ok && r < n) ? src[(int64_t)r * ld + col] : 0.f;
  }
}
// ... centred in fp64 and rounded once on their way into LDS (zero outside the matrix)
__device__ __forceinline__ void hsic_stage(float (*dst)[HLD], int n, int col, bool col_ok, double mu, int k0, int rsub, const float (&v)[HBK / 2]) {
#pragma unroll
  for (int i = 0; i < HBK / 2; ++i) {
    const int r = k0 + rsub + 2 * i;
    dst[rsub + 2 * i][col] = (col_ok && r < n) ? (float)((double)v[i] - mu) : 0.f;
  }
}

// grid (total tiles of the launch), block 256 = 2 x 2 waves of 64 x 64 (2 x 2 MFMA tiles of 32 x 32)
__global__ __launch_bounds__(256, 2) void cka_hsic_kernel(HsicBatch batch, double* __restrict__ part) {
  __shared__ float xs[2][HBK][HLD];
  __shared__ float ys[2][HBK][HLD];
  __shared__ double red[4];
  const int tile = blockIdx.x;
  int pi = 0;
  while (pi + 1 < batch.count && tile >= batch.tile_start[pi + 1]) ++pi;
  const HsicProd& pr = batch.p[pi];
  int t = tile - batch.tile_start[pi], ti, tj;
  if (pr.sym) {
    const int nt = (pr.hx + HT - 1) / HT;
    ti = 0;
    while (t >= nt - ti) { t -= nt - ti; ++ti; }
    tj = ti + t;
  } else {
    const int ny = (pr.hy + HT - 1) / HT;
    ti = t / ny;
    tj = t - ti * ny;
  }
  const int n = pr.n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  // loader: thread -> column (tid & 127), rows (tid >> 7) + 2i
  const int lcol = tid & (HT - 1), rsub = tid >> 7;
  const int cx = ti * HT + lcol, cy = tj * HT + lcol;
  const bool okx = cx < pr.hx, oky = cy < pr.hy;
  const double mux = okx ? pr.mx[cx] : 0.0, muy = oky ? pr.my[cy] : 0.0;
  const float* xsrc = pr.x;
  const float* ysrc = pr.y;

  f32x16 acc[2][2];
  f32x16 acc2[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[a][b][e] = 0.f; acc2[a][b][e] = 0.f; }
    }

  float vx[HBK / 2], vy[HBK / 2];
  hsic_fetch(xsrc, pr.ldx, n, cx, okx, 0, rsub, vx);
  hsic_fetch(ysrc, pr.ldy, n, cy, oky, 0, rsub, vy);
  const int steps = (n + HBK - 1) / HBK;
  const int steps_per_chunk = HSIC_CHUNK / HBK;
  const int ar = lane & 31, ak = lane >> 5;   // operand map of 32x32x2: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    hsic_stage(xs[buf], n, lcol, okx, mux, s * HBK, rsub, vx);
    hsic_stage(ys[buf], n, lcol, oky, muy, s * HBK, rsub, vy);
    __syncthreads();
    if (s + 1 < steps) {
      hsic_fetch(xsrc, pr.ldx, n, cx, okx, (s + 1) * HBK, rsub, vx);
      hsic_fetch(ysrc, pr.ldy, n, cy, oky, (s + 1) * HBK, rsub, vy);
    }
#pragma unroll
    for (int kk = 0; kk < HBK; kk += 2) {
      const float a0 = xs[buf][kk + ak][wm * 64 + ar], a1 = xs[buf][kk + ak][wm * 64 + 32 + ar];
      const float b0 = ys[buf][kk + ak][wn * 64 + ar], b1 = ys[buf][kk + ak][wn * 64 + 32 + ar];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if ((s + 1) % steps_per_chunk == 0 || s + 1 == steps) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          acc2[a][b] += acc[a][b];
          acc[a][b] = 0.f;
        }
    }
    // the next stage writes the other buffer; the barrier above already ordered every read of it
  }
  double sq = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int e = 0; e < 16; ++e) sq += (double)acc2[a][b][e] * (double)acc2[a][b][e];
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
  if (lane == 0) red[wave] = sq;
  __syncthreads();
  if (tid == 0) {
    const double v = (red[0] + red[1]) + (red[2] + red[3]);
    part[tile] = (pr.sym && ti != tj) ? 2.0 * v : v;
  }
}

// grid (products), block 256
__global__ __launch_bounds__(256) void cka_hsic_finish_kernel(const double* __restrict__ part, HsicBatch batch, double* __restrict__ out) {
  __shared__ double sm[256];
  const int p = blockIdx.x;
  const int t0 = batch.tile_start[p], t1 = batch.tile_start[p + 1];
  double a = 0.0;
  for (int t = t0 + threadIdx.x; t < t1; t += 256) a += part[t];
  sm[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[p] = sm[0];
}

static bool hsic_valid(const mafed_cka_product& q) {
  return q.X && q.Y && q.mean_x && q.mean_y && q.n > 0 && q.hx > 0 && q.hy > 0 && q.ldx >= q.hx && q.ldy >= q.hy && q.n <= INT32_MAX &&
         q.hx <= INT32_MAX && q.hy <= INT32_MAX;
}
static int hsic_sym(const mafed_cka_product& q) {
  return q.X == q.Y && q.mean_x == q.mean_y && q.hx == q.hy && q.ldx == q.ldy;
}

}  // namespace mafed

using namespace mafed;

extern "C" int mafed_cka_pool(const float* const* hidden_host, int L, int B, int S, int P, int h, const int64_t* attention_mask, int T,
                              const int64_t* rows, int64_t n, float* out, void* stream) {
  MAFED_CHECK_ARG(hidden_host && attention_mask && out && L > 0 && L <= POOL_MAX_LAYERS && B >= 0 && h > 0 && P >= 0 && T >= 0 && P + T <= S &&
                      n >= (rows ? 1 : B),
                  "cka_pool: bad arguments (L=%d B=%d S=%d P=%d T=%d h=%d n=%lld)", L, B, S, P, T, h, (long long)n);
  if (B == 0) return MAFED_OK;
  PoolLayers lay;
  for (int i = 0; i < L; ++i) {
    MAFED_CHECK_ARG(hidden_host[i], "cka_pool: hidden state %d is NULL", i);
    lay.p[i] = hidden_host[i];
  }
  launch(K_SMALL, 4.0 * B * L * (double)(P + T) * h, cka_pool_kernel, dim3(B, L, 2), dim3(256), 0, as_stream(stream), lay, S, P, h,
         attention_mask, T, rows, n, out);
  MAFED_CHECK_LAUNCH("cka_pool");
  return MAFED_OK;
}

extern "C" size_t mafed_cka_stats_workspace_bytes(int64_t G, int64_t n, int64_t h) {
  return (size_t)(G * cdiv(n, STAT_ROWS) * h) * sizeof(double);
}

extern "C" int mafed_cka_stats(const float* X, int64_t G, int64_t n, int64_t h, int64_t ldx, int64_t set_stride, double* mean,
                               double* row_sqnorm, void* workspace, size_t workspace_bytes, void* stream) {
  MAFED_CHECK_ARG(X && mean && G > 0 && n > 0 && h > 0 && ldx >= h && (G == 1 || set_stride >= (n - 1) * ldx + h) && G <= 65535,
                  "cka_stats: bad arguments (G=%lld n=%lld h=%lld ldx=%lld)", (long long)G, (long long)n, (long long)h, (long long)ldx);
  const size_t need = mafed_cka_stats_workspace_bytes(G, n, h);
  if (!workspace || workspace_bytes < need) {
    set_error("cka_stats: workspace %zu < %zu", workspace_bytes, need);
    return MAFED_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int64_t chunks = cdiv(n, STAT_ROWS);
  MAFED_CHECK_ARG(chunks <= 65535, "cka_stats: n=%lld too large", (long long)n);
  double* part = (double*)workspace;
  launch(K_SMALL, 4.0 * G * n * h, cka_colsum_kernel, dim3((unsigned)cdiv(h, 64), (unsigned)chunks, (unsigned)G), dim3(256), 0, st, X, n, h, ldx,
         set_stride, part);
  MAFED_CHECK_LAUNCH("cka_stats(colsum)");
  launch(K_SMALL, 8.0 * G * chunks * h, cka_mean_kernel, dim3((unsigned)cdiv(h, 256), (unsigned)G), dim3(256), 0, st, (const double*)part,
         (int)chunks, n, h, mean);
  MAFED_CHECK_LAUNCH("cka_stats(mean)");
  if (row_sqnorm) {
    MAFED_CHECK_ARG(cdiv(n, 4) <= INT32_MAX, "cka_stats: n too large");
    launch(K_SMALL, 4.0 * G * n * h, cka_rownorm_kernel, dim3((unsigned)cdiv(n, 4), (unsigned)G), dim3(256), 0, st, X, n, h, ldx, set_stride,
           (const double*)mean, row_sqnorm);
    MAFED_CHECK_LAUNCH("cka_stats(rownorm)");
  }
  return MAFED_OK;
}

extern "C" size_t mafed_cka_hsic_workspace_bytes(const mafed_cka_product* products, int count) {
  size_t t = 0;
  for (int i = 0; i < count; ++i) t += (size_t)hsic_tiles((int)products[i].hx, (int)products[i].hy, hsic_sym(products[i]));
  return t * sizeof(double);
}

extern "C" int mafed_cka_hsic(const mafed_cka_product* products, int count, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  MAFED_CHECK_ARG(count >= 0 && (count == 0 || (products && out)), "cka_hsic: bad arguments");
  for (int i = 0; i < count; ++i)
    MAFED_CHECK_ARG(hsic_valid(products[i]), "cka_hsic: product %d has bad shape / pointers (n=%lld hx=%lld hy=%lld)", i,
                    (long long)products[i].n, (long long)products[i].hx, (long long)products[i].hy);
  const size_t need = mafed_cka_hsic_workspace_bytes(products, count);
  if (count && (!workspace || workspace_bytes < need)) {
    set_error("cka_hsic: workspace %zu < %zu", workspace_bytes, need);
    return MAFED_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  double* part = (double*)workspace;
  for (int i0 = 0; i0 < count; i0 += HSIC_MAX_BATCH) {
    HsicBatch bt;
    bt.count = count - i0 < HSIC_MAX_BATCH ? count - i0 : HSIC_MAX_BATCH;
    bt.tile_start[0] = 0;
    double flop = 0.0;
    for (int j = 0; j < bt.count; ++j) {
      const mafed_cka_product& q = products[i0 + j];
      HsicProd& d = bt.p[j];
      d.x = q.X; d.y = q.Y; d.mx = q.mean_x; d.my = q.mean_y; d.ldx = q.ldx; d.ldy = q.ldy;
      d.n = (int)q.n; d.hx = (int)q.hx; d.hy = (int)q.hy; d.sym = hsic_sym(q);
      bt.tile_start[j + 1] = bt.tile_start[j] + hsic_tiles(d.hx, d.hy, d.sym);
      flop += d.sym ? (double)q.n * q.hx * q.hx : 2.0 * q.n * q.hx * q.hy;
    }
    for (int j = bt.count + 1; j <= HSIC_MAX_BATCH; ++j) bt.tile_start[j] = bt.tile_start[bt.count];
    launch(K_GEMM_F32, flop, cka_hsic_kernel, dim3((unsigned)bt.tile_start[bt.count]), dim3(256), 0, st, bt, part);
    MAFED_CHECK_LAUNCH("cka_hsic");
    launch(K_SMALL, 8.0 * bt.tile_start[bt.count], cka_hsic_finish_kernel, dim3((unsigned)bt.count), dim3(256), 0, st, (const double*)part, bt,
           out + i0);
    MAFED_CHECK_LAUNCH("cka_hsic(finish)");
    part += bt.tile_start[bt.count];
  }
  return MAFED_OK;
}
