/*
 * mafed_hip.h -- C-ABI of the MI355X-native (gfx950) MAFED training hot path.
 *
 * The reference (MalvinaNikandrou/mafed) is pure Python and has no FFI of its own; the arithmetic of its
 * per-step path lives in torch / transformers / flash-attn calls.  Each entry point below names the reference
 * call site it replaces (paths relative to the reference checkout; "tf:" = transformers
 * models/gpt_neox/modeling_gpt_neox.py).  INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; row-major, contiguous unless an ld is given
 *   - `stream` is a hipStream_t passed as void*; every launch goes on it; nothing allocates, synchronises or throws
 *   - return 0 on success, a negative MAFED_E* code otherwise (mafed_last_error_string() has the detail)
 *   - dtype arguments use mafed_dtype; the fp32 residual stream / statistics / gradients of parameters are float
 *   - parameter-gradient outputs ACCUMULATE (+=): the host zeroes the flat gradient buffer once per
 *     accumulation window (Lightning accumulate_grad_batches semantics, mafed/train.py:286)
 */
#ifndef MAFED_HIP_H
#define MAFED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MAFED_F32 = 0, MAFED_BF16 = 1 } mafed_dtype;

enum {
  MAFED_OK = 0,
  MAFED_EINVAL = -1,   /* bad shape / alignment / unsupported combination */
  MAFED_ELAUNCH = -2,  /* hipLaunch / hipGetLastError failed */
  MAFED_EWORKSPACE = -3 /* workspace too small */
};

/* GEMM epilogues (mafed_gemm.epilogue) */
enum {
  MAFED_EPI_NONE = 0,
  MAFED_EPI_GELU = 1,     /* C = gelu_erf(acc + bias); aux (if non-NULL) receives the pre-activation acc + bias */
  MAFED_EPI_GELU_BWD = 2, /* C = (acc) * gelu_erf'(aux) ; aux = saved pre-activation, same dtype as C */
  MAFED_EPI_QUICK_GELU = 3, /* C = x * sigmoid(1.702 x), x = acc + bias: MLP activation of the frozen CLIP vision tower (clip:338-350) */
  MAFED_EPI_RES1_BF16 = 0x100, /* flag, OR-ed in: res1 points at bf16 data (the attention branch output under bf16 autocast) */
  MAFED_EPI_NO_PERSISTENT = 0x200, /* flag, OR-ed in: THIS call keeps off the one-block-per-CU persistent kernels (a product that runs beside a
                                      long-resident kernel of another stream, e.g. a collective); per call, no process-wide state */
  MAFED_EPI_TICKETED = 0x400 /* flag, OR-ed in: if THIS call takes a persistent kernel over more than one round of the CUs, the blocks draw
                                their tiles from per-XCD queues instead of walking a static schedule (tolerates CUs held by other streams'
                                kernels: 1.2 - 1.3x instead of 1.7 - 1.9x with 8 - 32 CUs taken; costs a free chip ~2 %) */
};

int mafed_version(void);
const char* mafed_last_error_string(void);

/* ---- dense contractions -------------------------------------------------------------------------------
 * C[M,N] = op(A)[M,K] . op(B)[K,N]  (+ bias[n]) -> epilogue -> (+ res1 + res2) (+ beta * C_old)
 *   transA == 0: A stored [M,K] (lda >= K)     transA == 1: A stored [K,M] (lda >= M)
 *   transB == 0: B stored [K,N] (ldb >= N)     transB == 1: B stored [N,K] (ldb >= K)   (nn.Linear weight)
 * in_dtype MAFED_BF16: MFMA v_mfma_f32_16x16x32_bf16, fp32 accumulate; MAFED_F32: exact fp32 FMA path (parity mode).
 * c_dtype may be F32 or BF16; res1/res2 are fp32 [M,N] (ld = ldc) or NULL (res1 may be bf16: MAFED_EPI_RES1_BF16); beta != 0 requires c_dtype F32.
 * Replaces: every nn.Linear on the path -- query_key_value / dense (tf:192-193,204,233), dense_h_to_4h /
 * dense_4h_to_h + GELU (tf:38-49), vision_embed_tokens (mafed/model/vl_pythia.py:226-234,270), embed_out (:213,310),
 * their autograd backward (dX = dY.W, dW += dY^T.X), and the parallel-residual add (tf:271-274) via res1/res2.
 */
int mafed_gemm(mafed_dtype in_dtype, int transA, int transB, int64_t M, int64_t N, int64_t K,
               const void* A, int64_t lda, const void* B, int64_t ldb,
               void* C, int64_t ldc, mafed_dtype c_dtype,
               const float* bias, int epilogue, void* aux,
               const float* res1, const float* res2, float beta, void* stream);

/* mafed_gemm that also accumulates the column sums of the stored C: colsum[n] += sum_m C[m,n] (fp32 [N], may be NULL;
 * beta must be 0).  This is the bias gradient of the nn.Linear whose output gradient this GEMM produces
 * (dense_h_to_4h.bias from the GELU' epilogue of dX = dY.W2), fused into the epilogue of the MFMA kernel instead of
 * a second pass over C; where the selected kernel has no fused form the library runs mafed_colsum itself. */
int mafed_gemm_colsum(mafed_dtype in_dtype, int transA, int transB, int64_t M, int64_t N, int64_t K,
                      const void* A, int64_t lda, const void* B, int64_t ldb,
                      void* C, int64_t ldc, mafed_dtype c_dtype,
                      const float* bias, int epilogue, void* aux,
                      const float* res1, const float* res2, float beta, float* colsum, void* stream);

/* Grouped form: n independent products with the same operand layouts (transA / transB), input and output types, each with its own
 * shape, leading dimensions and epilogue (fields as the arguments of mafed_gemm_colsum).  Where every problem tiles the persistent
 * MFMA kernel they run as ONE launch whose tile space is the concatenation of theirs -- the parameter gradients dW += dY^T.X of several
 * layers fill the 256 CUs in whole rounds that way, without split-K -- otherwise as n launches.  Same results as n mafed_gemm_colsum
 * calls.  Replaces: the per-parameter weight-gradient products of autograd's Linear backward (tf:38-49,192-236), batched across layers. */
typedef struct mafed_gemm_problem {
  int64_t M, N, K;
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  void* C; int64_t ldc;
  const float* bias; int epilogue; void* aux;
  const float* res1; const float* res2; float beta; float* colsum;
  float* sumsq; /* NULL, or 16 floats: sumsq[k] += the squares of part of the STORED C (fp32 C only; which tile adds to which of the 16 slots
                   is unspecified, their total is sum C^2).  The weight-gradient products of a window's last micro-batch leave the squared
                   norm of the final gradient here, so that the clip's norm pass (mafed_gradnorm_partial, 1.2 GB at 410M) skips the
                   matrices (mafed/train.py:288 clip_grad_norm_). */
} mafed_gemm_problem;
int mafed_gemm_grouped(mafed_dtype in_dtype, int transA, int transB, mafed_dtype c_dtype,
                       const mafed_gemm_problem* problems, int n, void* stream);

/* out[n] += sum_m X[m,n]   (bias gradients; X dtype bf16/f32, out fp32 accumulated with one atomic per column per
 * 256-row block; N, ldx multiples of 4).  workspace is unused (kept for ABI stability; workspace_bytes may be 0). */
size_t mafed_colsum_workspace_bytes(int64_t M, int64_t N);
int mafed_colsum(const void* X, mafed_dtype dtype, int64_t M, int64_t N, int64_t ldx, float* out,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- LayerNorm (tf:243-244,313: nn.LayerNorm, eps 1e-5) ---------------------------------------------------
 * Dual-affine: with use_parallel_residual both LNs of a layer normalise the same tensor (tf:261,272), so x is read
 * once and two outputs are written.  Pass w2 = b2 = y2 = NULL for a single LN (final_layer_norm).
 * x fp32 [rows,h]; y1/y2 in out_dtype; mean/rstd fp32 [rows] saved for backward (may be NULL for inference).
 */
int mafed_layernorm_fwd(const float* x, int64_t rows, int h, float eps,
                        const float* w1, const float* b1, void* y1,
                        const float* w2, const float* b2, void* y2,
                        mafed_dtype out_dtype, float* mean, float* rstd, void* stream);
/* dx = LN'(dy1;w1) + LN'(dy2;w2) + dres ; optional dx_lp = dx cast to dy_dtype (the next GEMM's operand).
 * dy1/dy2 in dy_dtype (dy2, w2, dw2, db2 NULL for single LN); dres fp32 [rows,h] or NULL (the residual-stream
 * gradient flowing around the layer); dx fp32 [rows,h] (may alias dres).  dw1/db1/dw2/db2 fp32 [h], accumulated.
 * Optional fused distillation-gradient injection (the hidden state this LN normalises is a distilled one,
 * mafed/methods/distillation.py:237-249 backward): if teacher != NULL,
 *   dx[row,:] += inj_mul * inj_scale[row_class] * (x - teacher)   with row_class from (row % S): <P image, text-valid, pad=none
 * where inj_scale_dev = {lang, vision} = d(loss)/d(sum_lang d), d(loss)/d(sum_vision d) (coeff * weight / count * upstream grad,
 * left on the device by the loss algebra) and inj_mul = 2/h (MSE).
 * A NEGATIVE inj_mul selects the cosine-distance loss of mafed_distill_fwd(cosine = 1) instead (distillation_loss="cosine",
 * mafed/methods/distillation.py:226-235):
 *   dx[row,:] += |inj_mul| * inj_scale[row_class] * d/dx [ 1 - x.t / sqrt((x.x + 1e-12)(t.t + 1e-12)) ]     (inj_mul = -1 for the plain loss) */
size_t mafed_layernorm_bwd_workspace_bytes(int64_t rows, int h);
int mafed_layernorm_bwd(const void* dy1, const void* dy2, mafed_dtype dy_dtype,
                        const float* x, const float* mean, const float* rstd,
                        const float* w1, const float* w2, int64_t rows, int h,
                        const float* dres, float* dx, void* dx_lp,
                        float* dw1, float* db1, float* dw2, float* db2,
                        const float* teacher, const int64_t* attention_mask, int S, int P, int T,
                        const float* inj_scale_dev /* [2] device: {lang, vision} or NULL */, float inj_mul /* host factor, e.g. 2/h */,
                        float* dxsum_a, float* dxsum_b /* optional fp32 [h]: += column sums of dx (bias grads of the layer below) */,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The same backward in two calls, so that the parameter reduction can run on another stream, off the dX chain (the caller orders
 * it behind the row kernel and keeps `workspace` private to this pair):
 *   mafed_layernorm_bwd_rows    dx, dx_lp and the per-block partials of dw / db (/ column sums of dx when want_dxsum) into workspace
 *   mafed_layernorm_bwd_params  workspace -> dw1, db1 (dw2, db2), dxsum_a / dxsum_b; pass dw2 / dxsum_* exactly as "dual" / want_dxsum were */
int mafed_layernorm_bwd_rows(const void* dy1, const void* dy2, mafed_dtype dy_dtype, const float* x, const float* mean, const float* rstd,
                             const float* w1, const float* w2, int64_t rows, int h, const float* dres, float* dx, void* dx_lp,
                             const float* teacher, const int64_t* attention_mask, int S, int P, int T, const float* inj_scale_dev,
                             float inj_mul, int want_dxsum, void* workspace, size_t workspace_bytes, void* stream);
int mafed_layernorm_bwd_params(int64_t rows, int h, float* dw1, float* db1, float* dw2, float* db2, float* dxsum_a, float* dxsum_b,
                               const void* workspace, size_t workspace_bytes, void* stream);
/* mafed_layernorm_bwd / mafed_layernorm_bwd_rows with the teacher rows of the injection read where they are stored (a slab of a resident
 * teacher cache, FeatureDistillation.build_teacher_cache) instead of from a dense fp32 [rows,h] copy of the batch's rows:
 *   teacher        [n,S,h] in teacher_dtype: MAFED_F32, or MAFED_BF16 (widened to fp32 at the load; needs an 8-byte aligned base)
 *   sample_index   int32 [rows / S] device, or NULL: the teacher row of token (b, s) is teacher[(sample_index ? sample_index[b] : b) * S + s]
 *                  (offset formed in 64 bits); x, dy, the mask and the row class keep using b.  Entries must lie in [0, n); an index
 *                  without a teacher is MAFED_EINVAL.
 * Every other argument as in the call without the suffix, which is this one with (teacher, MAFED_F32, NULL): same kernel, same bits. */
int mafed_layernorm_bwd_indexed(const void* dy1, const void* dy2, mafed_dtype dy_dtype,
                                const float* x, const float* mean, const float* rstd,
                                const float* w1, const float* w2, int64_t rows, int h,
                                const float* dres, float* dx, void* dx_lp,
                                float* dw1, float* db1, float* dw2, float* db2,
                                const void* teacher, mafed_dtype teacher_dtype, const int* sample_index,
                                const int64_t* attention_mask, int S, int P, int T,
                                const float* inj_scale_dev, float inj_mul, float* dxsum_a, float* dxsum_b,
                                void* workspace, size_t workspace_bytes, void* stream);
int mafed_layernorm_bwd_rows_indexed(const void* dy1, const void* dy2, mafed_dtype dy_dtype, const float* x, const float* mean,
                                     const float* rstd, const float* w1, const float* w2, int64_t rows, int h, const float* dres, float* dx,
                                     void* dx_lp, const void* teacher, mafed_dtype teacher_dtype, const int* sample_index,
                                     const int64_t* attention_mask, int S, int P, int T, const float* inj_scale_dev, float inj_mul,
                                     int want_dxsum, void* workspace, size_t workspace_bytes, void* stream);

/* ---- attention (tf:154-236 eager path / flash-attn-2 wheel, README.md:16) ------------------------------------
 * qkv: [B,S,H,3,D] exactly as the fused query_key_value GEMM leaves it (per-head {q,k,v} interleave, tf:204-207).
 * Partial rotary (first rot dims, NeoX rotate_half pairing, position = row index, tf:111-151) is applied to q and k
 * on load; rot_cos/rot_sin fp32 [S, rot/2].  Fully causal over S, plus key-padding from attention_mask [B,T]
 * (int64, 1 = valid; LEFT padded so invalid keys are the contiguous range [P, P+pad_b)); P = S - T image keys are
 * always valid.  softmax in fp32; scale = D^-0.5.  out [B,S,H*D] in dtype; lse fp32 [B,H,S] (natural log).
 * dtype BF16: MFMA kernels (D in {64,128}); F32: exact parity kernels (D <= 256).
 */
int mafed_attn_fwd(const void* qkv, mafed_dtype dtype, int B, int S, int H, int D, int rot,
                   const float* rot_cos, const float* rot_sin, const int64_t* attention_mask, int T,
                   void* out, float* lse, void* stream);
/* dqkv [B,S,H,3,D] (dtype) <- d(out); inverse rotation applied to dq, dk.  delta fp32 [B,H,S] scratch. */
int mafed_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, mafed_dtype dtype,
                   int B, int S, int H, int D, int rot, const float* rot_cos, const float* rot_sin,
                   const int64_t* attention_mask, int T, void* dqkv, float* delta, void* stream);
/* mafed_attn_bwd that also accumulates dqkv_colsum[3*H*D] += sum over the B*S rows of dqkv: the gradient of
 * query_key_value.bias (tf:192), folded inside the resident MFMA kernels (one run of atomics per block) instead of a
 * second pass over dqkv; other paths run mafed_colsum themselves.  dqkv_colsum may be NULL. */
int mafed_attn_bwd_colsum(const void* qkv, const void* out, const void* dout, const float* lse, mafed_dtype dtype,
                          int B, int S, int H, int D, int rot, const float* rot_cos, const float* rot_sin,
                          const int64_t* attention_mask, int T, void* dqkv, float* delta, float* dqkv_colsum, void* stream);

/* ---- KV-cached greedy decode (mafed/model/vqa_cont_learner.py:260-277 calls
 * generate(max_new_tokens=10, use_cache=False), i.e. ten full forwards over the 256 + T prefix) ---------------------
 * One new query per sample against every earlier key.  qkv_prefix [B,S0,H,3,D] is what the prefill's fused QKV GEMM wrote
 * (k un-rotated; rotation applied on load, position = key index, as in mafed_attn_fwd); qkv_new [B,cap,H,3,D] holds one
 * row per generated token, row t being the current one (its q is the query, position S0 + t; keys = S0 + t + 1).
 * rot_cos / rot_sin cover at least S0 + t + 1 positions.  attention_mask [B,T] is the PROMPT's key-padding mask (P = S0 - T
 * image keys and all generated keys are valid).  out [B,H*D] in dtype. */
int mafed_attn_decode(const void* qkv_prefix, int S0, const void* qkv_new, int cap, int t, mafed_dtype dtype,
                      int B, int H, int D, int rot, const float* rot_cos, const float* rot_sin,
                      const int64_t* attention_mask, int T, void* out, void* stream);

/* The same step over a cache of ROTATED keys: qkv_prefix's k part has been rotated in place once behind the prefill
 * (mafed_rotate_k_rows), rows < t of qkv_new by the steps that appended them; this call rotates row t's k (as written by the QKV
 * GEMM), uses it and writes it back rotated.  A step then loads k and v only -- no rotary partner chunk, no cos / sin rows per key
 * (two thirds of the on-load form's load instructions).  rot % 16 == 0, D in {64, 128, 256}.  Same result as mafed_attn_decode up to
 * the rounding of the stored rotated keys (bf16 cache: one more bf16 rounding on the first `rot` dims of k). */
int mafed_attn_decode_prerot(const void* qkv_prefix, int S0, void* qkv_new, int cap, int t, mafed_dtype dtype,
                             int B, int H, int D, int rot, const float* rot_cos, const float* rot_sin,
                             const int64_t* attention_mask, int T, void* out, void* stream);
/* k part of every row of a [B,S,H,3,D] qkv tensor rotated in place for its position (row index within the sample): turns a prefill's
 * fused-QKV output into the pre-rotated cache of mafed_attn_decode_prerot.  rot % 16 == 0. */
int mafed_rotate_k_rows(void* qkv, mafed_dtype dtype, int B, int S, int H, int D, int rot, const float* rot_cos, const float* rot_sin,
                        void* stream);

/* ---- fused decode layer (mafed/model/vqa_cont_learner.py:260-277 -> HF greedy search over
 * mafed/model/vl_pythia.py's GPT-NeoX stack, one row per sample and step) ----------------------------------------------
 * A GPT-NeoX layer (parallel residual) of a decode step in three launches: mafed_decode_ln_qkv_fc1, mafed_attn_decode_prerot,
 * mafed_decode_out.  bf16 weights [N, K] row-major, bf16 activations, fp32 residual stream x [M, h], M <= 64 rows.
 * mafed_decode_supported: 1 if the shape is served (h % 256 == 0 with h / 256 in {1, 2, 3, 4, 8}, n1 % 32 == 0, ceil(M/16) * h/256 <= 16). */
int mafed_decode_supported(int M, int h, int n1);
/* qkv_out[m, 0:3h] = LN1(x[m]) . wqkv^T + bqkv   (row m at qkv_out + m * qkv_ld elements: the K/V cache row of this step)
 * a_out[m, 0:n1]   = gelu(LN2(x[m]) . w1^T + b1) (erf form)
 * Both LayerNorms (two-pass statistics in fp32, output rounded to bf16 like mafed_layernorm_fwd) are computed in the prologue. */
int mafed_decode_ln_qkv_fc1(const float* x, int M, int h, float eps, const float* ln1_w, const float* ln1_b, const float* ln2_w,
                            const float* ln2_b, const void* wqkv, const float* bqkv, void* qkv_out, int64_t qkv_ld, const void* w1,
                            const float* b1, int n1, void* a_out, void* stream);
/* out[m, 0:N] = LN(x[m]) . w^T (+ bias, may be NULL): the final LayerNorm folded into the LM head's product (the last two launches of a
 * decode step as one).  bf16 w [N, h] and out (row stride ldo elements); N % 32 == 0; M, h as mafed_decode_supported(M, h, 32). */
int mafed_decode_ln_linear(const float* x, int M, int h, float eps, const float* ln_w, const float* ln_b, const void* w, const float* bias,
                           int64_t N, void* out, int64_t ldo, void* stream);
/* x_out[m] = x[m] + bd + b2 + ao[m] . wd^T + act[m] . w2^T   (attention output projection and 4h -> h projection as one product over
 * the concatenated K = h + n1; x_out may alias x).  The K reduction is split over blocks; partial tiles are added in slice order by the
 * last block of a column group to arrive (no floating-point atomics: bit-identical from run to run).  workspace: at least
 * mafed_decode_out_workspace_bytes(M, h) bytes, ZERO-FILLED once before the first call (it holds the arrival counters, which every
 * launch leaves at zero again); one workspace per stream. */
size_t mafed_decode_out_workspace_bytes(int M, int h);
/* tools: device buffer of 8 int64 per workgroup that the next mafed_decode_out launches fill with wall-clock stamps (NULL = off) */
int mafed_decode_set_trace(void* buf);
int mafed_attn_decode_set_trace(void* buf);   /* the same for mafed_attn_decode_prerot's all-rows-in-flight kernel: 8 int64 per (batch, head) */
int mafed_decode_out(const float* x, float* x_out, int M, int h, int n1, const void* ao, const void* act, const void* wd,
                     const float* bd, const void* w2, const float* b2, void* workspace, size_t workspace_bytes, void* stream);
/* M > 64 (up to 256 rows: B = 32 samples x 8 beams): mafed_decode_ln_qkv_fc1 and mafed_decode_out run the rows in blocks of 64, each
 * block exactly as a call with those 64 rows (the same kernels and bits; decode_out's workspace is the 64-row one, re-used in order).
 * mafed_decode_ln_linear stays at M <= 64. */

/* ---- beam search over a shared-prefix KV cache (model.generate(num_beams=k), HF GenerationMixin._beam_search semantics) ---------
 * Per sample: one prefill; per layer the prefix [B,S0,H,3,D] (pre-rotated keys) shared by the sample's k beams and the generated rows
 * [B*k,cap,H,3,D] (slot r writes its row t at [r, t]); an int32 ancestry table anc [B*k,cap] names the slot holding row j of beam r's
 * history.  A reorder rewrites anc only (anc'[r,j] = anc[parent(r),j] for j < t, anc'[r,t] = r): no K/V is copied.  k <= 8.
 *
 * mafed_beam_candidates: logits [B*kin, V] (row stride ldl, fp32 or bf16) and running scores [B*kin] -> per sample the top 2k of
 * log_softmax(logits[row]) + score[row] over its kin rows x V tokens, best first: out_score [B,2k] fp32, out_token [B,2k] int64,
 * out_parent [B,2k] int32 (row within the sample).  Order: score descending; equal scores go to the lower flat index row * V + token. */
int mafed_beam_candidates(const void* logits, mafed_dtype dtype, int64_t ldl, const float* score, int B, int kin, int V, int k,
                          float* out_score, int64_t* out_token, int* out_parent, void* stream);
/* One beam-search step's bookkeeping, one workgroup per sample (HF 5.x _beam_search with one eos id, eos < 0: none): candidates among
 * the first k ranks that emit eos (or every one at step == cap - 1) join the finished set with score / (step + 1)^length_penalty, the
 * k best finished hypotheses are kept best first; the first k candidates that did not finish continue (run_score, next_token, the
 * rows of anc / hist rewritten); early_stopping 0 / 1 / 2 = False / True / "never" with HF's stop heuristic, after which a sample is
 * `done` (its set is final; its beams feed pad).  The *_in / *_out pairs are distinct buffers (ping-pong between steps).  fin_tok
 * [B,k,cap] int64 holds the hypotheses' generated tokens padded with `pad`, fin_score [B,k] (-1e9 = empty), fin_len [B,k] (0 = empty). */
int mafed_beam_update(const float* cand_score, const int64_t* cand_token, const int* cand_parent, int B, int k, int step, int cap,
                      int eos, int pad, int early_stopping, float length_penalty, float* run_score, const int* anc_in, int* anc_out,
                      const int64_t* hist_in, int64_t* hist_out, const int64_t* fin_tok_in, int64_t* fin_tok_out,
                      const float* fin_score_in, float* fin_score_out, const int* fin_len_in, int* fin_len_out, int* done,
                      int64_t* next_token, void* stream);
/* Decode attention of the k beams of every sample over the layout above: one workgroup per (sample, head) serves the k query rows
 * (row t of each beam slot, position S0 + t), reads the sample's prefix K/V once for all of them, rows j < t through anc and row t
 * from the beam's own slot (its key rotated, used and written back rotated, as mafed_attn_decode_prerot does).  attention_mask
 * [B,T] per sample.  rot % 16 == 0, D in {64, 128, 256}.  out [B*k, H*D]. */
int mafed_attn_decode_beam(const void* qkv_prefix, int S0, void* qkv_new, int cap, int t, mafed_dtype dtype, int B, int k,
                           const int* anc, int H, int D, int rot, const float* rot_cos, const float* rot_sin,
                           const int64_t* attention_mask, int T, void* out, void* stream);

/* ---- shared-image prefill (generate / sample with image_index; DESIGN.md section 4c''') ------------------------------------------
 * B prompts over N distinct images.  The prompt is [P image | T text], fully causal with arange positions, so the image rows' K / V
 * depend on the image alone: they are computed once per image into qkv_img [N,P,H,3,D] (k un-rotated, as the QKV GEMM wrote it) and
 * the text rows qkv_txt [B,T,H,3,D] attend them through image_index [B] (int64, values in [0, N); NULL = identity, N == B).
 * mafed_attn_suffix_fwd computes exactly rows P .. P+T-1 of mafed_attn_fwd on the assembled [B, P+T] sequence: query j of prompt b
 * sits at position P + j and sees the P keys of its image and text keys 0 .. j of its own prompt, minus the left-padding range of
 * attention_mask [B,T]; partial rotary on load (position = key index, rot_cos / rot_sin cover >= P + T positions); softmax in fp32,
 * scale D^-0.5.  A query at a padded position, or of a prompt whose text is all padding, still attends the image keys.
 * F32: exact kernel, D <= 256.  BF16: MFMA kernel over 64-key tiles for D in {64, 128, 256} with rot in {0, 16, 32, 64} (16-byte
 * aligned tensors), the exact kernel on bf16 data otherwise.  out [B,T,H*D] in dtype.  Index values are clamped into [0, N). */
int mafed_attn_suffix_fwd(const void* qkv_img, const int64_t* image_index, int N, int P, const void* qkv_txt, int T, mafed_dtype dtype,
                          int B, int H, int D, int rot, const float* rot_cos, const float* rot_sin, const int64_t* attention_mask,
                          void* out, void* stream);
/* The decode cache's prefix from the two stores, every layer in one launch: out [L, B*(P+T), W] = per prompt the P rows of image
 * image_index[b] from qkv_img [L, N*P, W], then its own T rows from qkv_txt [L, B*T, W].  A plain 16-byte-per-lane copy: the row
 * size (W elements of dtype) is a multiple of 16 bytes, the tensors are 16-byte aligned. */
int mafed_prefix_gather(const void* qkv_img, const void* qkv_txt, const int64_t* image_index, int L, int N, int B, int P, int T, int64_t W,
                        mafed_dtype dtype, void* out, void* stream);

/* ---- candidate scoring (model.score; DESIGN.md section 4c'''') -------------------------------------------------------------------
 * C candidate answers of A tokens each behind one prefilled prompt.  qkv_prefix [B,S0,H,3,D] holds the prompt's fused-QKV rows (S0 =
 * P image + T text positions, k un-rotated, as the QKV GEMM wrote them), qkv_cand [B,C,A,H,3,D] the candidates' rows.
 * mafed_attn_cand_fwd: out[b,c,j] = row S0 + j of mafed_attn_fwd on the assembled [prefix b | candidate (b,c)] sequence of length
 * S0 + A under the mask [attention_mask[b] | ones(A)]: the query sits at position S0 + j and sees the P = S0 - T image keys, the prefix
 * text keys that the left-padding mask [B,T] leaves and keys 0 .. j of its own candidate, nothing of another candidate; partial rotary
 * on load (position = key index: candidate key j is at S0 + j for every c; rot_cos / rot_sin cover >= S0 + A positions); softmax in
 * fp32, scale D^-0.5.  T < S0: key 0 is an image key, so a prompt whose text is all padding still attends its image and no row is
 * empty.  F32: exact kernel, D <= 256.  BF16: MFMA kernel for D in {64, 128, 256} with rot in {0, 16, 32, 64} on 16-byte aligned
 * tensors -- the C*A rows of one (b,h) are one query axis cut into 64-row tiles, each prefix key tile staged once per query tile --
 * the exact kernel on bf16 data otherwise.  out [B,C,A,H*D] in dtype. */
int mafed_attn_cand_fwd(const void* qkv_prefix, int S0, const void* qkv_cand, int C, int A, mafed_dtype dtype, int B, int H, int D, int rot,
                        const float* rot_cos, const float* rot_sin, const int64_t* attention_mask, int T, void* out, void* stream);
/* out[r] = logits[row(r), target[r]] - logsumexp(logits[row(r), :]) in fp32, row(r) = logits_row[r] (NULL: r): several outputs may
 * read one logits row (the C candidates' first token from the prompt's last position).  logits fp32 or bf16, row stride ldl elements;
 * target [R] int64: < 0 gives 0 (a masked position), >= V gives NaN.  Fixed reduction order: the same bits on every call, whatever R. */
int mafed_token_logprob(const void* logits, mafed_dtype dtype, int64_t ldl, const int* logits_row, const int64_t* target, int R, int64_t V,
                        float* out, void* stream);
/* out[r] = sum over the j with mask[r,j] != 0 (mask NULL: all) of token_logprob[r,j], in ascending j; mean != 0 divides by their
 * number; a row without a token gives -inf.  token_logprob fp32 [R,A], mask int64 [R,A]. */
int mafed_score_reduce(const float* token_logprob, const int64_t* mask, int R, int A, int mean, float* out, void* stream);

/* ---- sampled decoding (model.sample) -------------------------------------------------------------------------------------------
 * One launch draws one token per row: what transformers.GenerationMixin._sample does per step with TemperatureLogitsWarper,
 * TopKLogitsWarper, TopPLogitsWarper and MinPLogitsWarper (in that order), softmax and torch.multinomial, plus the eos / pad tail of
 * the greedy pick.  logits [R, V] fp32 or bf16, row stride ldl elements, V <= 65536.  With z = logit / temperature (> 0):
 *   top_k  (0 = off)       keep z >= the k-th largest z; ties at the threshold are all kept
 *   top_p  in (0, 1]       over the top-k survivors: keep z >= z*, the largest value with mass{z > z*} < top_p * mass(survivors) <=
 *                          mass{z >= z*}.  A tie on the cut is kept whole (TopPLogitsWarper keeps an order-dependent part of it).
 *   min_p  in [0, 1)       keep z >= z_max + log(min_p)
 * and with p_i = exp(z_i - z_max) / Z over the kept set the token is the first kept id, ascending, whose inclusive cumulative
 * probability exceeds u.  u = uniforms[row] when uniforms != NULL; otherwise Philox4x32-10 with key = (low, high) half of *seed (one
 * word in DEVICE memory, read by the kernel: a captured launch sees the value the word holds at replay) and counter = (row, step, 0,
 * 0), u = ((x0 >> 8) + 0.5) * 2^-24 evaluated in fp32.  Masses are 64-bit integers (floor(exp(z - z_max) * 2^47)), so a row's result is the same bits
 * on every run and does not depend on R or on the other rows.
 * unfinished (may be NULL; int64 [R], read and written): a row whose flag is 0 emits `pad` (logprob 0, kept 0); a drawn `eos`
 * (eos < 0: none) clears the row's flag.  token int64 [R]; logprob (may be NULL) fp32 [R], the log-probability of the drawn token under
 * the kept, renormalised distribution; kept (may be NULL) int32 [R], the size of the kept set. */
int mafed_sample_token(const void* logits, mafed_dtype dtype, int64_t ldl, int R, int V, float temperature, int top_k, float top_p,
                       float min_p, const uint64_t* seed, int step, const float* uniforms, int64_t* unfinished, int eos, int pad,
                       int64_t* token, float* logprob, int* kept, void* stream);

/* ---- online EWC penalty (mafed/methods/ewc.py:105-127) -------------------------------------
 * The reference's compute_regularization over named_parameters(), on the flat fp32 buffers:
 *   fwd: out[0] = beta * out[0] + half_lambda * sum_i fisher[i] * (p[i] - p_old[i])^2     (half_lambda = 0.5 * reg_lambda;
 *        beta = 1 chains the per-task terms of the non-online variant, ewc.py:124-126)
 *   bwd: grad[i] += coef_dev[0] * lambda * fisher[i] * (p[i] - p_old[i])                  (coef_dev = d loss / d penalty)
 * Deterministic two-stage reduction; workspace from mafed_ewc_workspace_bytes. */
size_t mafed_ewc_workspace_bytes(int64_t n);
int mafed_ewc_penalty_fwd(const float* p, const float* p_old, const float* fisher, int64_t n, float half_lambda, float beta,
                          float* out, void* workspace, size_t workspace_bytes, void* stream);
int mafed_ewc_penalty_bwd(const float* p, const float* p_old, const float* fisher, int64_t n, float lambda,
                          const float* coef_dev, float* grad, void* stream);

/* ---- A-GEM gradient projection (Chaudhry et al., 2019) ---------------------------------------
 * On flat fp32 buffers, g = the step's gradient, r = the gradient of one replay-memory batch at the same parameters:
 *   dots:    stats4 = {dot = sum g r, rsq = sum r r, alpha, violated} with alpha = dot / rsq and violated = 1 if dot < 0 and rsq > 0,
 *            else alpha = 0 and violated = 0.  A non-finite dot or rsq gives alpha = NaN, violated = 1 (nothing is hidden: g' and its
 *            norm are then non-finite and the optimiser's guard skips the step).  Per-block partials in the workspace
 *            (mafed_agem_workspace_bytes), folded in double by one block: no atomics, the same bits on every run.
 *   project: out[i] = g[i] - alpha * r[i] with alpha read from stats4[2] on the device; alpha == 0 copies g bit for bit (r is not read).  out may
 *            alias r (or g).  sumsq_partials (or NULL) receives mafed_agem_blocks(n) sum-of-squares partials of out, which
 *            mafed_gradnorm_finish folds into the clip norm.
 * n == 0: dots writes stats4 = {0, 0, 0, 0}, project writes one zero partial. */
size_t mafed_agem_workspace_bytes(int64_t n);
int mafed_agem_blocks(int64_t n);
int mafed_agem_dots(const float* g, const float* r, int64_t n, float* stats4, void* workspace, size_t workspace_bytes, void* stream);
int mafed_agem_project(const float* g, const float* r, float* out, int64_t n, const float* stats4, float* sumsq_partials, void* stream);

/* ---- GEM gradient constraints (Lopez-Paz & Ranzato, 2017) ------------------------------------------
 * On flat fp32 buffers, g = the step's gradient, refs[0 .. K) = the gradients of one memory batch per finished task at the same
 * parameters, 1 <= K <= 8.  refs is a HOST array of K device pointers; they travel by value in the kernel arguments.
 *   gram:    gram64[(K + 1) x (K + 1)] (device, fp64, symmetric to the bit) = sum_i x_a[i] x_b[i] with x_0 = g, x_k = refs[k - 1].  Products and
 *            per-thread sums in fp32, (K + 1)(K + 2) / 2 partials per block in the workspace (mafed_gem_workspace_bytes), folded in
 *            double by one block: no atomics, the same bits on every run.
 *   solve:   q_k = gram[0][k], P = gram[1..K][1..K] + eps I.  Every q_k >= 0: stats12 = 0.  Else v = argmin 1/2 v'Pv + q'v subject to
 *            v_k >= margin, exactly, by enumerating the supports in fp64; stats12[0 .. 7] = v (zeros behind K),
 *            stats12[8] = violated (0 / 1), stats12[9] = size of the chosen support, stats12[10 .. 11] = 0.  A non-finite Gram entry
 *            (or no feasible support) gives v_k = NaN and violated = 1: nothing is hidden.
 *   project: stats12[8] == 0: out = g bit for bit and no ref is read.  Else out[i] = g[i] + sum_k stats12[k] refs[k][i], one fma per
 *            k in ascending order.  out may alias g or any ref.  sumsq_partials (or NULL) receives mafed_gem_blocks(n) sum-of-squares
 *            partials of out, which mafed_gradnorm_finish folds into the clip norm.
 * n == 0: gram writes a zero matrix, project writes one zero partial. */
size_t mafed_gem_workspace_bytes(int64_t n, int K);
int mafed_gem_blocks(int64_t n);
int mafed_gem_gram(const float* g, const float* const* refs, int K, int64_t n, double* gram64, void* workspace, size_t workspace_bytes,
                   void* stream);
int mafed_gem_solve(const double* gram64, int K, float margin, float eps, float* stats12, void* stream);
int mafed_gem_project(const float* g, const float* const* refs, int K, float* out, int64_t n, const float* stats12, float* sumsq_partials,
                      void* stream);

/* ---- Synaptic Intelligence (Zenke, Poole, Ganguli 2017) ------------------------------------------
 * On flat fp32 buffers laid out like the parameters p: the step gradient g, the path integral w, the importance omega, the anchor
 * and the stash pair (stash_g, stash_p).
 *   stash:       stash_g = g and stash_p = p, bit copies.  With omega and anchor (both or neither): g[i] += two_c * omega[i] * (p[i] -
 *                anchor[i]) in place; without them g is only read.  sumsq_partials receives mafed_si_blocks(n) sum-of-squares
 *                partials of the g it leaves (for mafed_gradnorm_finish), pen_partials as many partials of sum omega (p - anchor)^2
 *                (zeros without omega).  No atomics: the same bits on every run.
 *   penalty_finish: out[0] = c * sum of n_partials penalty partials, folded in double in a fixed order by one block.
 *   accumulate:  w[i] -= stash_g[i] * (p[i] - stash_p[i]) where p[i] != stash_p[i]; an element that did not move keeps w[i] bit for
 *                bit, whatever stash_g[i] holds (a select: a skipped step's non-finite gradient leaves no trace).
 *   consolidate: omega[i] = max(omega[i] + w[i] / ((p[i] - anchor[i])^2 + xi), 0) by true division (a negative sum gives +0, a NaN
 *                stays), then anchor[i] = p[i] and w[i] = 0.  xi > 0.
 * n == 0: stash writes one zero partial of each kind, accumulate and consolidate do nothing. */
int mafed_si_blocks(int64_t n);
int mafed_si_stash(float* g, const float* p, const float* omega, const float* anchor, int64_t n, float two_c, float* stash_g,
                   float* stash_p, float* sumsq_partials, float* pen_partials, void* stream);
int mafed_si_penalty_finish(const float* pen_partials, int n_partials, float c, float* out, void* stream);
int mafed_si_accumulate(const float* stash_g, const float* stash_p, const float* p, float* w, int64_t n, void* stream);
int mafed_si_consolidate(const float* p, float* anchor, float* w, float* omega, int64_t n, float xi, void* stream);

/* ---- Memory Aware Synapses (Aljundi et al. 2018) --------------------------------------------------
 * On flat fp32 buffers laid out like the parameters p: the gradient g, the importance accumulator acc, the importance omega, the anchor.
 *   accumulate:  acc[i] = fma(weight, |g[i]|, acc[i])  (one batch of the importance pass; the sign of g, a -0.0 included, is dropped).
 *   consolidate: first != 0: omega[i] = inv_seen * acc[i] (omega is not read);  else omega[i] = alpha * omega[i] + (1 - alpha) * inv_seen *
 *                acc[i] as fma(alpha, omega, k acc) with k = (1 - alpha) * inv_seen folded in double.  Then anchor[i] = p[i], acc[i] = 0.
 *                inv_seen > 0, 0 <= alpha <= 1.
 *   penalty:     g[i] += two_c * omega[i] * (p[i] - anchor[i]) in place: the arithmetic, the partials (mafed_mas_blocks(n) of each kind,
 *                == mafed_si_blocks(n)) and the bits of mafed_si_stash with omega and anchor, without the stash.  sumsq_partials goes to
 *                mafed_gradnorm_finish, pen_partials to mafed_si_penalty_finish.  No atomics: the same bits on every run.
 * n == 0: penalty writes one zero partial of each kind, accumulate and consolidate do nothing. */
int mafed_mas_blocks(int64_t n);
int mafed_mas_accumulate(const float* g, float* acc, int64_t n, float weight, void* stream);
int mafed_mas_consolidate(float* acc, float* omega, const float* p, float* anchor, int64_t n, float inv_seen, float alpha, int first,
                          void* stream);
int mafed_mas_penalty(float* g, const float* p, const float* omega, const float* anchor, int64_t n, float two_c, float* sumsq_partials,
                      float* pen_partials, void* stream);

/* ---- PackNet (Mallya & Lazebnik 2018) ---------------------------------------------------------------
 * On flat buffers laid out like the fp32 parameters p: the gradient g, the anchor, the bf16 shadow of p (raw bits; NULL = none) and the
 * byte-wide owner map (owner[i] = the task that trained element i).  Base pointers must be 16-byte aligned.
 *   mask_grad:  g[i] = owner[i] == task ? g[i] : +0.0 in place; sumsq_partials receives mafed_packnet_blocks(n) sum-of-squares partials
 *               of the g it leaves, for mafed_gradnorm_finish.  No atomics: the same bits on every run.  n == 0: one zero partial.
 *   hold:       where owner[i] != task: p[i] = anchor[i], shadow[i] = bf16(anchor[i]) (round to nearest even).  Nothing else is written.
 *   view:       where owner[i] > k: p[i] = +0.0, shadow[i] = 0.  Nothing else is written.
 * The prune is an exact k-th-smallest selection per segment, a three-pass radix select (11 + 10 + 10 bits) on the 31-bit pattern of |p|
 * (-0 equals +0, a NaN sorts above +inf).  segments = device int64 [n_segments][2] = {offset, length} into the flat buffers, any alignment,
 * length < 2^32; an element outside [0, n) is ignored.  One launch covers all segments, grid (blocks_per_segment, n_segments).
 *   hist:   pass 0, 1, 2: hist[s][bin] (uint32 [n_segments][2048], cleared by the call) = number of elements of segment s with
 *           owner == task whose bits above the pass's digit equal the prefix in state; integer atomics only.
 *   scan:   one block per segment.  Pass 0 also derives m = number of elements with owner == task and k = floor(fraction * m) in IEEE
 *           double.  Walks the bins to the one that holds rank k and writes the extended prefix and the remaining rank.
 *           state = int64 [n_segments][4] = {prefix, rank, active (k > 0), unused}; stats = int64 [n_segments][4] = {m, k, pruned, tau},
 *           tau = the pattern of the k-th smallest |p| (0 while k == 0), written by pass 2.
 *   apply:  every element with owner == task and |p| <= tau (as patterns): p = +0.0, anchor = +0.0, owner = task + 1, shadow = 0;
 *           stats[s][2] = their number (ties at tau are all pruned, so it may exceed k).
 * 0 <= task <= 254, 0 <= fraction <= 1.  The host reads nothing back. */
int mafed_packnet_blocks(int64_t n);
int mafed_packnet_mask_grad(float* g, const uint8_t* owner, int64_t n, int task, float* sumsq_partials, void* stream);
int mafed_packnet_hold(float* p, void* shadow, const uint8_t* owner, const float* anchor, int64_t n, int task, void* stream);
int mafed_packnet_view(float* p, void* shadow, const uint8_t* owner, int64_t n, int k, void* stream);
int mafed_packnet_hist(const float* p, const uint8_t* owner, int64_t n, const int64_t* segments, int n_segments, int blocks_per_segment,
                       int task, int pass, const int64_t* state, uint32_t* hist, void* stream);
int mafed_packnet_scan(const uint32_t* hist, int n_segments, int pass, double fraction, int64_t* state, int64_t* stats, void* stream);
int mafed_packnet_apply(float* p, void* shadow, uint8_t* owner, float* anchor, int64_t n, const int64_t* segments, int n_segments,
                        int blocks_per_segment, int task, const int64_t* state, int64_t* stats, void* stream);

/* ---- task-vector model merging: task arithmetic, MagMax, TIES -------------------------------------------
 * On flat fp32 buffers laid out like the parameters: theta (the fine-tuned parameters), base (theta_0) and the streaming state.  Base
 * pointers must be 16-byte aligned.  tau = fl(theta - base), one IEEE subtraction; every sum, product and quotient below is rounded on its
 * own (no FMA), counts are integers: the same bits on every run.
 *   fold:       MAFED_MERGE_SUM: acc = fl(acc + tau).  MAFED_MERGE_MAGMAX: acc = |tau| > |acc| ? tau : acc (strict; a NaN tau never wins, a
 *               NaN acc never leaves).
 *   ties_hist:  pass 0, 1, 2 of the radix select of mafed_packnet_hist (same segments table, digits, 2048-bin histograms, state) on the
 *               31-bit pattern of |tau|, over every element of a segment.  The scan between two passes is mafed_packnet_scan with
 *               fraction = 1 - density: m = the segment's length, r = floor(fraction * m), tau_bits = the r-th smallest pattern.
 *   ties_fold:  with the state the third scan left: element i of a segment is kept iff r == 0 or pattern(|tau|) > tau_bits.  Kept and
 *               tau > 0: pos += tau, counts[2 i] += 1; kept and tau < 0: neg += tau, counts[2 i + 1] += 1 (byte counters: 255 folds at
 *               most); tau == 0 or NaN: nothing.  stats[s][2] = the number kept.  Elements outside every segment are not touched.
 *   apply:      d = acc (sum, magmax; neg and counts NULL) or, for MAFED_MERGE_TIES with acc = pos and s = fl(pos + neg):
 *               s > 0: pos / npos, s < 0: neg / nneg, else +0.0.  p = fl(base + fl(scaling * d)); shadow (bf16 bits, or NULL) = bf16(p),
 *               round to nearest even.
 * The host reads nothing back. */
enum { MAFED_MERGE_SUM = 0, MAFED_MERGE_MAGMAX = 1, MAFED_MERGE_TIES = 2 };
int mafed_merge_fold(const float* theta, const float* base, float* acc, int64_t n, int rule, void* stream);
int mafed_merge_ties_hist(const float* theta, const float* base, int64_t n, const int64_t* segments, int n_segments, int blocks_per_segment,
                          int pass, const int64_t* state, uint32_t* hist, void* stream);
int mafed_merge_ties_fold(const float* theta, const float* base, float* pos, float* neg, uint8_t* counts, int64_t n, const int64_t* segments,
                          int n_segments, int blocks_per_segment, const int64_t* state, int64_t* stats, void* stream);
int mafed_merge_apply(float* p, void* shadow, const float* base, const float* acc, const float* neg, const uint8_t* counts, int64_t n, int rule,
                      float scaling, void* stream);

/* ---- representation-drift analysis: per-layer, per-modality linear CKA (mafed/analysis/) --------------------------
 * Modality pooling of one forward's hidden states (mafed/analysis/get_average_CKA_per_layer.py:107-118): for sample b and
 * layer l (hidden_host[l] = hidden_states[l + 1], fp32 [B, S, h], S = P + T)
 *   out[0, l, rows[b], :] = mean of hidden[b, 0:P, :]                          (image)
 *   out[1, l, rows[b], :] = mean of hidden[b, S - txt_len : S, :]              (text, txt_len = sum_t attention_mask[b, t])
 * out fp32 [2, L, n, h]; rows int64 [B] or NULL (row b; a row outside [0, n) drops the sample); txt_len == 0 gives NaN, as the reference's mean of an empty slice.
 * fp64 sums in a fixed order.  L <= 64; hidden_host is a HOST array of L device pointers. */
int mafed_cka_pool(const float* const* hidden_host, int L, int B, int S, int P, int h, const int64_t* attention_mask, int T,
                   const int64_t* rows, int64_t n, float* out, void* stream);

/* Column means and centred row norms of G feature sets X_g [n, h] (row stride ldx, set g at X + g * set_stride), fp64:
 *   mean[g, c] = sum_r X_g[r, c] / n            row_sqnorm[g, r] = sum_c (X_g[r, c] - mean[g, c])^2   (row_sqnorm may be NULL)
 * Replaces: the centring of feature_space_linear_cka (mafed/analysis/cka.py:133-134) and its debiased estimator's
 * sum_squared_rows (cka.py:144-147).  Deterministic (fixed-order fp64 reductions). */
size_t mafed_cka_stats_workspace_bytes(int64_t G, int64_t n, int64_t h);
int mafed_cka_stats(const float* X, int64_t G, int64_t n, int64_t h, int64_t ldx, int64_t set_stride, double* mean,
                    double* row_sqnorm, void* workspace, size_t workspace_bytes, void* stream);

/* One product of mafed_cka_hsic: X [n, hx] (row stride ldx) and Y [n, hy] (row stride ldy), fp32, with their fp64 column
 * means (mafed_cka_stats).  A product whose X, mean_x, hx and ldx equal Y, mean_y, hy and ldy is a self term. */
typedef struct mafed_cka_product {
  const float* X; const double* mean_x; int64_t ldx; int64_t hx;
  const float* Y; const double* mean_y; int64_t ldy; int64_t hy;
  int64_t n;
} mafed_cka_product;

/* Batched centred cross-Gram Frobenius norm, out[p] = ||(X_p - 1 mean_x^T)^T (Y_p - 1 mean_y^T)||_F^2 (fp64 [count]).
 * Replaces: np.linalg.norm(features_x.T.dot(features_y)) ** 2 and the two self-similarity norms of
 * feature_space_linear_cka (mafed/analysis/cka.py:136-138).  fp32-input MFMA on operands centred in fp64, the MFMA
 * accumulators flushed into second-level fp32 ones every 4096 rows, C never stored, fp64 squares; results are bitwise the
 * same for every batch composition.
 * n, hx, hy < 2^31.  workspace: mafed_cka_hsic_workspace_bytes(products, count) bytes (host-side query). */
size_t mafed_cka_hsic_workspace_bytes(const mafed_cka_product* products, int count);
int mafed_cka_hsic(const mafed_cka_product* products, int count, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- replay-memory selection in a feature space ---------------------------------------------------------------
 * Replaces: the memory sub-sampling of mafed/methods/replay.py and distillation.py:182-209 (rng.choice) by the two standard
 * selections, herding (iCaRL) and k-center greedy, over X fp32 [n, d] (row stride ldx >= d) with its fp64 column mean
 * (mafed_cka_stats).  k greedy picks from one call, two launches per pick, nothing read back in between.
 *   dist(i, v) = sum_j (X[i, j] - v[j])^2, fp32, direct differences; its bits depend on row i's contents and on v only.
 *   A row is eligible while it is not picked and its score is not NaN; ties go to the lowest row; when no row is left the
 *   remaining picks are -1 and their values NaN.
 *   herding:  r_0 = mean; pick t minimises dist(i, fp32(r_t)); values[t] = that minimum; r_{t+1} = (r_t + mean) - X[p_t] in fp64.
 *   k-center: pick 0 is herding's pick 0 (values[0] = its distance to the mean); m_i = +inf; for t >= 1
 *             m_i = min(m_i, dist(i, X[p_{t-1}])), pick t maximises m_i, values[t] = that maximum.
 *   last_scores[i] (may be NULL): the score row i had in the last pick, picked rows included.
 * picks int64 [k], values fp32 [k], 1 <= k <= n < 2^31 - 1.  16-byte loads when d % 4 == 0, ldx % 4 == 0 and X is 16-byte
 * aligned; any d >= 1 otherwise.  Deterministic.  workspace: mafed_select_workspace_bytes(n, d) bytes, 16-byte aligned. */
enum { MAFED_SELECT_HERDING = 0, MAFED_SELECT_KCENTER = 1 };
size_t mafed_select_workspace_bytes(int64_t n, int64_t d);
int mafed_select_greedy(const float* X, int64_t n, int64_t d, int64_t ldx, const double* mean, int mode, int64_t k, int64_t* picks,
                        float* values, float* last_scores, void* workspace, size_t workspace_bytes, void* stream);

/* ---- embedding + concat (mafed/model/vl_pythia.py:282-283) ---------------------------------------------------
 * h0[b, :P] = image[b] ; h0[b, P:] = embed_in[input_ids[b]]  -> fp32 [B,P+T,h].  image in img_dtype [B,P,h]. */
int mafed_embed_concat_fwd(const void* image, mafed_dtype img_dtype, const float* embed_in, const int64_t* input_ids,
                           int B, int P, int T, int h, int64_t V, float* h0, void* stream);
/* d_image[b] = dh0[b,:P] (img_dtype) ; d_embed_in[input_ids[b,t]] += dh0[b,P+t] (fp32 atomics) */
int mafed_embed_concat_bwd(const float* dh0, const int64_t* input_ids, int B, int P, int T, int h, int64_t V,
                           void* d_image, mafed_dtype img_dtype, float* d_embed_in, void* stream);

/* ---- per-sample-normalised shifted cross-entropy (mafed/model/vl_pythia.py:44-96) ---------------------------
 * logits [B,T,V] (text positions only), labels int64 [B,T]; row (b,t) predicts labels[b,t+1]; ignore_index -100;
 * loss = mean_b( sum_t ce[b,t] / max(count_b, 1e-13) ).  lse fp32 [B,T] saved.  loss_out fp32 [1]. */
int mafed_ce_fwd(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V,
                 float* lse, float* row_loss /* [B,T] scratch */, float* loss_out, void* stream);
/* mafed_ce_fwd whose loss becomes NaN when the device flag *poison_flag is non-zero: the row-sparse LM head (mafed_label_rows) raises
 * its overflow flag when a sample has more labelled positions than the caller's hint promised -- rows were dropped, the loss would be
 * silently wrong -- and the step then fails loudly (NaN loss, caught by every trainer) without a host synchronisation. */
int mafed_ce_fwd_guarded(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V,
                         float* lse, float* row_loss, float* loss_out, const int* poison_flag, void* stream);
/* dlogits[b,t,:] = gloss * (softmax - onehot) / (B * count_b) for valid rows, 0 otherwise (incl. t = T-1).
 * gloss_dev: device scalar (upstream dL/dloss).  dlogits may alias logits. */
int mafed_ce_bwd(const void* logits, mafed_dtype dtype, const int64_t* labels, const float* lse, int B, int T, int64_t V,
                 const float* gloss_dev, void* dlogits, void* stream);

/* ---- squared-norm head objective (the MAS importance pass) ----------------------------------
 * logits, labels, the shift, V % 4 == 0 and the alignment as for mafed_ce_fwd; a row (b,t) is labelled when t < T-1 and labels[b,t+1] != -100.
 * The label values are not used otherwise.
 *   fwd: rowsq fp32 [B,T] = sum_c logits[b,t,c]^2 on labelled rows, 0 elsewhere; out fp32 [1] = J = mean_b( sum_t rowsq[b,t] /
 *        max(count_b, 1e-13) ).  poison_flag (may be NULL): a non-zero device flag turns J into NaN (mafed_ce_fwd_guarded).
 *   bwd: dlogits[b,t,:] = dloss * 2 logits[b,t,:] / (B * max(count_b, 1e-13)) on labelled rows, exact zeros elsewhere, in `dtype`; no
 *        forward output is needed.  dloss_dev: device scalar (upstream dL/dJ).  dlogits: a buffer of its own.
 * No atomics, no workspace: the same bits on every call. */
int mafed_sqnorm_fwd(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V, float* rowsq, float* out,
                     const int* poison_flag, void* stream);
int mafed_sqnorm_bwd(const void* logits, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V, const float* dloss_dev,
                     void* dlogits, void* stream);

/* ---- LwF head loss: the cross-entropy above + temperature-softened logit distillation, one pass per direction ----
 * student, teacher: logits [B,T,V] of the same head rows in `dtype` (F32 or BF16; the teacher's are a frozen model's); labels as above.
 * With p^tau_x = softmax(x / tau), tau > 0, per labelled row (shifted label != -100, never the last position):
 *   CE = lse(s) - s[lab]
 *   KD = KL(p^tau_t || p^tau_s) = sum_c p^tau_t[c] (t[c] - s[c]) / tau - lse(t / tau) + lse(s / tau)
 * each summed per sample / max(count_b, 1e-13) and averaged over B like mafed_ce_fwd; out3 fp32 [3] = { CE + lambda tau^2 KD, CE, KD }.
 * lse3 fp32 [3, B*T] = { lse(s), lse(s / tau), lse(t / tau) } saved for the backward (0 on unlabelled rows, which are not read);
 * row_ce, row_kd: fp32 [B*T] scratch.  poison_flag (may be NULL): a non-zero device flag turns out3[0] into NaN (mafed_ce_fwd_guarded).
 * Every exponential is max-subtracted; student == teacher gives KD == 0.0 exactly; tau == 1 gives lse3[0] == lse3[1] bit for bit.
 * V % 4 == 0; fp32 logits 16-byte, bf16 logits 8-byte aligned.  No atomics, no workspace: the same bits on every call. */
int mafed_ce_kd_fwd(const void* student, const void* teacher, mafed_dtype dtype, const int64_t* labels, int B, int T, int64_t V,
                    float tau, float lambda, float* lse3, float* row_ce, float* row_kd, float* out3, const int* poison_flag,
                    void* stream);
/* dlogits[b,t,:] = g_b (softmax(s) - onehot(lab)) + g_b lambda tau (p^tau_s - p^tau_t), g_b = gloss / (B * count_b), for labelled rows;
 * 0 otherwise (incl. t = T-1).  gloss_dev: device scalar (upstream dL/dloss).  dlogits: `dtype` [B,T,V], a buffer of its own. */
int mafed_ce_kd_bwd(const void* student, const void* teacher, mafed_dtype dtype, const int64_t* labels, const float* lse3, int B, int T,
                    int64_t V, float tau, float lambda, const float* gloss_dev, void* dlogits, void* stream);

/* ---- DER++ head loss: the cross-entropy above + the squared distance to stored answer logits, one pass per direction ----
 * No reference call site: the reference names the method (the `_der_` checkpoint suffix, mafed/utils/eval_utils.py:23) and ships none.
 * student: logits [B,T,V] in `dtype` (F32 or BF16); labels as above.  store: [n_mem, A, V] of `dtype`, contiguous: the logits a model
 * gave on the answer rows of the n_mem replay samples when they were stored.  mem_index int64 [B]: the stored sample of batch row b.
 * A labelled row (b,t) (shifted label != -100, never the last position) is paired with z = store[mem_index[b], j, :], j = the number
 * of labelled rows of sample b in front of t (its rank).  Per labelled row:
 *   CE  = lse(s) - s[lab]
 *   MSE = (1 / V) sum_c (s[c] - z[c])^2           (fp32; the difference first, so s == z gives exactly 0)
 * each summed per sample / max(count_b, 1e-13) and averaged over B like mafed_ce_fwd; out3 fp32 [3] = { beta CE + alpha MSE, CE, MSE }.
 * lse fp32 [B*T] saved for the backward (0 on unlabelled rows, which are not read); row_ce, row_mse: fp32 [B*T] scratch.
 * poison_flag (may be NULL): a non-zero device flag turns out3[0] into NaN (mafed_ce_fwd_guarded).
 * A labelled row with mem_index[b] outside [0, n_mem) or j >= A has no stored row: nothing of the store is read for it and its MSE
 * (and with it out3[0] and out3[2]) is NaN -- the step fails loudly, without a host synchronisation.
 * The log-sum-exp is mafed_ce_fwd's own: with store row == student row and beta == 1, out3[0] == out3[1], lse and the gradient are
 * mafed_ce_fwd's / mafed_ce_bwd's bit for bit on the labelled rows; alpha == 0 likewise.
 * V % 4 == 0, n_mem > 0, A > 0, alpha and beta finite; fp32 tensors 16-byte, bf16 tensors 8-byte aligned.  No atomics, no workspace:
 * the same bits on every call. */
int mafed_ce_mse_fwd(const void* student, const void* store, mafed_dtype dtype, const int64_t* labels, const int64_t* mem_index, int B,
                     int T, int64_t V, int64_t n_mem, int A, float alpha, float beta, float* lse, float* row_ce, float* row_mse,
                     float* out3, const int* poison_flag, void* stream);
/* dlogits[b,t,:] = g_b (beta (softmax(s) - onehot(lab)) + alpha (2 / V) (s - z)), g_b = gloss / (B * count_b), for labelled rows; 0
 * otherwise (incl. t = T-1); NaN on a labelled row without a stored row.  gloss_dev: device scalar (upstream dL/dloss).  dlogits:
 * `dtype` [B,T,V], a buffer of its own. */
int mafed_ce_mse_bwd(const void* student, const void* store, mafed_dtype dtype, const int64_t* labels, const int64_t* mem_index,
                     const float* lse, int B, int T, int64_t V, int64_t n_mem, int A, float alpha, float beta, const float* gloss_dev,
                     void* dlogits, void* stream);

/* ---- MAFED per-modality masked distillation (mafed/methods/distillation.py:124-166, 226-257) -----------------
 * s, t: fp32 [B,S,h] student / frozen-teacher hidden state of one layer; attention_mask int64 [B,T]; P image tokens.
 * One pass serves both masks: out[4] = { sum_lang d, sum_vision d, n_lang, n_vision } with
 *   mse:    d[row] = sum((s-t)^2)/h                      (_compute_mse_distillation_loss, :237-249)
 *   cosine: d[row] = 1 - cos(s,t)  (CosineEmbeddingLoss target 1; aten's form: cos = st / sqrt((ss + 1e-12) (tt + 1e-12)), the epsilon on the SQUARED norms; :226-235)
 * Deterministic two-stage reduction (no float atomics).  workspace >= mafed_distill_workspace_bytes(B*S). */
size_t mafed_distill_workspace_bytes(int64_t rows);
int mafed_distill_fwd(const float* s, const float* t, const int64_t* attention_mask, int B, int S, int P, int h,
                      int cosine, float* out4, void* workspace, size_t workspace_bytes, void* stream);
/* ds (+)= g_lang[row] / g_vision[row] weighted gradient of the above:  coef_dev[2] = {c_lang, c_vision} where the
 * host/torch side already folded upstream grad * layer_coeff * distillation_coeff * modality weight / count.
 *   mse:    ds = c * 2/h * (s - t)
 *   cosine: ds = c * -( t/(|s||t|) - cos * s/|s|^2 )
 * accumulate != 0 adds into ds, else overwrites (rows of no modality get 0). */
int mafed_distill_bwd(const float* s, const float* t, const int64_t* attention_mask, int B, int S, int P, int h,
                      int cosine, const float* coef_dev, float* ds, int accumulate, void* stream);
/* CLS variant (:251-257): token 0 only, cosine, mean over batch -> out[1]; bwd with coef_dev[1] = upstream/B */
/* The scalar tail of distill() for every distilled layer in one launch (mafed/methods/distillation.py:105-122,147-162;
 * distillation_loss_weights.py:71-79): from sums[n_layers][4] = {sum_lang, sum_vis, n_lang, n_vis} (mafed_distill_fwd) and the device
 * vector layer_coeff[n_layers] (layer coefficient x distillation_coeff) it writes per_layer[l] = lw * sum_lang / n_lang + vw * sum_vis / n_vis,
 * modality[l] = {lang mean, vision mean}, loss = sum_l coeff[l] * per_layer[l], and inject[l] = d loss / d {sum_lang, sum_vis, ., .}
 * (the coefficients mafed_layernorm_bwd's fused injection takes, to be scaled by the upstream gradient of the loss).
 * modality_mode 0 "equal": lw = n_lang / (n_lang + n_vis); 1 "balanced": lw = lang_weight; 2 "adaptive": lw = lang_weight_vec[l]. */
int mafed_distill_combine(const float* sums, int n_layers, const float* layer_coeff_dev, int modality_mode, float lang_weight,
                          const float* lang_weight_vec_dev, float* loss_out, float* per_layer_out, float* modality_out,
                          float* inject_out, void* stream);

int mafed_distill_cls_fwd(const float* s, const float* t, int B, int S, int h, float* out1, void* stream);
int mafed_distill_cls_bwd(const float* s, const float* t, int B, int S, int h, const float* coef_dev, float* ds,
                          int accumulate, void* stream);
/* The four calls above with the teacher rows read where they are stored (one layer's slab of a resident teacher cache) instead of from
 * a dense fp32 [B,S,h] tensor:
 *   teacher        [n,S,h] in teacher_dtype: MAFED_F32, or MAFED_BF16 (each element widened to fp32 at the load, everything after the
 *                  load unchanged; needs h % 4 == 0 and an 8-byte aligned base).  A bf16 teacher IS the distillation target: the sums
 *                  and gradients are those of the rounded rows (relative rounding <= 2^-9 per element).
 *   sample_index   int32 [B] device, or NULL: the teacher row of token (b, s) is teacher[(sample_index ? sample_index[b] : b) * S + s]
 *                  (offset formed in 64 bits); s, ds, attention_mask and the row class keep using b.  Entries must lie in [0, n).
 * mafed_distill_fwd(s, t, ...) is mafed_distill_fwd_indexed(s, t, MAFED_F32, NULL, ...), and likewise the other three: the same kernel on
 * the same values, the same order of every sum. */
int mafed_distill_fwd_indexed(const float* s, const void* teacher, mafed_dtype teacher_dtype, const int* sample_index,
                              const int64_t* attention_mask, int B, int S, int P, int h, int cosine, float* out4,
                              void* workspace, size_t workspace_bytes, void* stream);
int mafed_distill_bwd_indexed(const float* s, const void* teacher, mafed_dtype teacher_dtype, const int* sample_index,
                              const int64_t* attention_mask, int B, int S, int P, int h, int cosine, const float* coef_dev,
                              float* ds, int accumulate, void* stream);
int mafed_distill_cls_fwd_indexed(const float* s, const void* teacher, mafed_dtype teacher_dtype, const int* sample_index,
                                  int B, int S, int h, float* out1, void* stream);
int mafed_distill_cls_bwd_indexed(const float* s, const void* teacher, mafed_dtype teacher_dtype, const int* sample_index,
                                  int B, int S, int h, const float* coef_dev, float* ds, int accumulate, void* stream);

/* ---- optimiser side -------------------------------------------------------------------------------------------
 * Global L2 norm of a flat fp32 gradient buffer (Lightning gradient_clip_val -> clip_grad_norm_, mafed/train.py:288):
 * out[0] = ||g||_2, out[1] = clip scale = min(1, max_norm / (norm + 1e-6)).  workspace >= gradnorm_workspace_bytes. */
size_t mafed_gradnorm_workspace_bytes(int64_t n);
int mafed_gradnorm_clip(const float* g, int64_t n, float max_norm, float* out2, void* workspace, size_t workspace_bytes,
                        void* stream);
/* The same norm in pieces: mafed_gradnorm_partial writes mafed_gradnorm_blocks(n) sum-of-squares partials of one range (call it as soon
 * as that range of the gradient is final, on the stream that finished it); mafed_gradnorm_finish folds n_partials of them (index
 * order) into out2 = {norm, clip scale}.  Replaces the single pass over the whole buffer at the start of the optimiser step. */
int mafed_gradnorm_blocks(int64_t n);
int mafed_gradnorm_partial(const float* g, int64_t n, float* partial_out, void* stream);
int mafed_gradnorm_finish(const float* partial, int n_partials, float max_norm, float* out2, void* stream);
/* HF-style AdamW on a flat segment (mafed/optim/adamw.py:86-111): m,v update; denom = sqrt(v) + eps (not bias
 * corrected); p -= lr*sqrt(1-b2^t)/(1-b1^t) * m/denom; then p -= lr*wd*p.  g is multiplied by clip_scale_dev[1]
 * (from mafed_gradnorm_clip) and by grad_mul (1/world for DDP means).  lr_dev: device scalar (scheduled lr).
 * step >= 1: bias corrections computed on the host from step (double).  step == 0: lr_dev points at three floats
 * {lr, 1-b1^t, sqrt(1-b2^t)} that the host refreshes before each launch -- the form a hipGraph replay needs.
 * If p_bf16 != NULL also writes the bf16 shadow copy used by the MFMA GEMMs.  The host keeps decayed and
 * non-decayed parameters in two contiguous segments of the flat buffer and calls this once per segment. */
int mafed_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2,
                     float eps, float weight_decay, int step, const float* clip_dev /* out2 of gradnorm or NULL */,
                     float grad_mul, void* p_bf16, void* stream);

/* mafed_adamw_step that also writes zeros over g in the same pass (optimizer.zero_grad() of the next accumulation window). */
int mafed_adamw_step_zero_grad(float* p, float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2,
                               float eps, float weight_decay, int step, const float* clip_scale_dev, float grad_mul, void* p_bf16,
                               void* stream);

/* General form: zeroes only the first `zero_n` elements of g (0 = none, n = all of it = mafed_adamw_step_zero_grad).  For the chunk of one
 * decoder layer -- [LayerNorm weights | the four weight matrices] -- the host passes the LayerNorm part: their gradients are accumulated
 * (+=) by the LayerNorm backward and need a zeroed buffer, the matrices' gradients are OVERWRITTEN by the first micro-batch's weight-
 * gradient GEMMs of the next window (beta = 0), so zero-writing them (1.2 GB per step at 410M) and re-reading them in those GEMMs'
 * epilogues is skipped.  Replaces optimizer.zero_grad() + AdamW.step (mafed/optim/adamw.py:50-113) for that chunk. */
int mafed_adamw_step_partial_zero(float* p, float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2,
                                  float eps, float weight_decay, int step, const float* clip_scale_dev, float grad_mul, void* p_bf16,
                                  int64_t zero_n, void* stream);

/* torch.optim.Adam (coupled L2) on a flat segment, torch 2.x single-tensor rule: g' = g*gs + wd*p; m = b1*m + (1-b1)*g';
 * v = b2*v + (1-b2)*g'^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps) -- eps AFTER the bias correction, decay in the
 * gradient (unlike mafed_adamw_step).  gs = grad_mul * clip_dev[1]; a negative clip scale skips the step (p, m, v untouched).
 * lr_dev / step / p_bf16 as in mafed_adamw_step; zero_n as in mafed_adamw_step_partial_zero (0 = g kept, n = all of g zeroed).  The betas
 * are double (torch's and mafed_optim_advance's): 1 - beta is formed in double, and step > 0 gives the device advance's corrections. */
int mafed_adam_step(float* p, float* g, float* m, float* v, int64_t n, const float* lr_dev, double beta1, double beta2, float eps,
                    float weight_decay, int step, const float* clip_dev, float grad_mul, void* p_bf16, int64_t zero_n, void* stream);
/* torch.optim.Adamax, same conventions: g' and m as in mafed_adam_step; u = max(b2*u, |g'| + eps); p -= lr/(1-b1^t) * m / u. */
int mafed_adamax_step(float* p, float* g, float* m, float* u, int64_t n, const float* lr_dev, double beta1, double beta2, float eps,
                      float weight_decay, int step, const float* clip_dev, float grad_mul, void* p_bf16, int64_t zero_n, void* stream);

/* Device-resident schedule (mafed/optim/sched.py:34-48 + the bias corrections of adamw.py:94-97): state_dev[0] = number of
 * optimiser steps taken so far; increments it to t and writes hyper3_dev = {base_lr * lambda(t-1), 1-b1^t, sqrt(1-b2^t)}
 * (double precision inside) for mafed_adamw_step(step = 0).  total_steps <= 0 means a constant learning rate. */
int mafed_optim_advance(int64_t* state_dev, double base_lr, int64_t warmup_steps, int64_t total_steps, double beta1, double beta2,
                        float* hyper3_dev, void* stream);

/* Guard of an optimiser step against a non-finite gradient (what a GradScaler does on the device): the gradient-norm kernels write the
 * clip scale out2[1] = -1 when the global norm is NaN / infinite (e.g. the poisoned loss of the row-sparse head's overflow flag);
 * mafed_adamw_step* given such a clip_dev leaves p, m, v and the bf16 shadow untouched (the zero_grad form still zeroes g),
 * mafed_gradnorm_finish_advance does not advance the step counter, and this form of mafed_optim_advance does not either when
 * clip_dev[1] < 0 (clip_dev may be NULL = unguarded).  The host sees the skipped step as a non-finite out2[0] / norm_log at its next
 * natural synchronisation.  Reference behaviour (mafed/optim/adamw.py:86-111 applied to NaN gradients) would corrupt every parameter. */
int mafed_optim_advance_guarded(int64_t* state_dev, double base_lr, int64_t warmup_steps, int64_t total_steps, double beta1, double beta2,
                                float* hyper3_dev, const float* clip_dev, void* stream);

/* sumsq16[k] += the squares of part of x (k = 0..15, their total += sum x^2): the unfused form of mafed_gemm_problem.sumsq, and the way
 * to put any fp32 range into the same 16 slots.  x 16-byte aligned. */
int mafed_sumsq_accumulate(const float* x, int64_t n, float* sumsq16, void* stream);
/* 1 if mafed_gemm_grouped would run these n products (dense operands) as ONE persistent launch that fills mafed_gemm_problem.sumsq from its
 * epilogue; 0 if the squares would cost a pass over C behind the product(s) (shapes the 256 x 256-tile kernel takes, groups that do not
 * fill the chip) -- a caller that has a cheaper way to the same norm (mafed_gradnorm_partial over a contiguous range) then skips sumsq. */
int mafed_gemm_grouped_fuses_sumsq(mafed_dtype in_dtype, int transA, int transB, mafed_dtype c_dtype, const int64_t* M, const int64_t* N,
                                   const int64_t* K, int n);

/* mafed_gradnorm_finish followed by mafed_optim_advance as ONE launch (both are single-thread tails on the optimiser step's critical
 * path); norm_log (or NULL) additionally receives the norm -- a slot the caller owns, e.g. for the step's log record, so that no
 * device copy of out2[0] is needed before the next step overwrites it.  Same arithmetic, bit for bit, as the two calls. */
int mafed_gradnorm_finish_advance(const float* partial, int n_partials, float max_norm, float* out2, float* norm_log, int64_t* state_dev,
                                  double base_lr, int64_t warmup_steps, int64_t total_steps, double beta1, double beta2, float* hyper3_dev,
                                  void* stream);

/* ---- small utilities --------------------------------------------------------------------------------------------- */
int mafed_cast(const void* src, mafed_dtype src_dtype, void* dst, mafed_dtype dst_dtype, int64_t n, void* stream);
/* dst [B,S,h] fp32 = zeros for the P image positions of every sample, src [B,S-P,h] for its text positions; dst_lp (bf16, optional): the
 * same rows in the compute dtype.  The start of the residual-stream gradient: only text positions feed the LM head (vl_pythia.py:310). */
int mafed_pad_text_rows(const float* src, int B, int S, int P, int h, float* dst, void* dst_lp, void* stream);
/* Row-sparse LM head (training): the rows of the [B,T] text block whose shifted label is a token (labels[b,t+1] != -100), at most
 * Rc-1 per sample, as a compact [B,Rc] problem for the same CE kernels: row_of_slot [B*Rc] (text row or -1), slot_of_row [B*T] (slot or
 * -1), labels_c [B,Rc] (slot n's label at n+1).  overflow[0] = 1 if a sample had more labelled rows than fit.  mafed_gather_rows moves
 * the rows either way: dst[r,:] = idx[r] >= 0 ? src[idx[r],:] : 0. */
int mafed_label_rows(const int64_t* labels, int B, int T, int Rc, int* row_of_slot, int* slot_of_row, int64_t* labels_c, int* overflow,
                     void* stream);
int mafed_gather_rows(const void* src, mafed_dtype dtype, const int* idx, int64_t n_out, int h, void* dst, void* stream);
/* Right padding of a text batch in one launch: ids / mask / labels [B,T] int64 -> [B,Tp] (Tp >= T) with id 0, mask 0 and label -100 at
 * positions T .. Tp-1.  labels / labels_out may both be NULL.  The engine's ``text_bucket`` policy uses it to make B * (P + Tp) a multiple
 * of the GEMM tile: positions appended BEHIND the text are invisible to every real query and carry no loss term. */
int mafed_pad_text_batch(const int64_t* ids, const int64_t* mask, const int64_t* labels, int B, int T, int Tp, int64_t* ids_out,
                         int64_t* mask_out, int64_t* labels_out, void* stream);
/* y = gelu_erf(x) elementwise (used by tests; the product path fuses GELU into mafed_gemm) */
int mafed_gelu(const void* x, void* y, mafed_dtype dtype, int64_t n, void* stream);

/* ---- frozen CLIP vision tower (mafed/model/vl_pythia.py:196-198, 453-475; clip: = transformers/models/clip/modeling_clip.py) ----
 * The tower is ``CLIPVisionModel`` called with output_hidden_states and cut at hidden_states[-2]; its Linear layers go through
 * mafed_gemm (fc1 with MAFED_EPI_QUICK_GELU), its LayerNorms through mafed_layernorm_fwd; the three entry points below are the rest.
 * mafed_patchify: im2col of the stride = kernel patch convolution (clip:148-154, 209-210): pixels [B,C,H,W] ->
 *   out [rows_out, k_pad], out[b * np + p][c * patch^2 + i * patch + j] = pixels[b][c][py * patch + i][px * patch + j]; columns
 *   >= C * patch^2 and rows >= B * np are zero (k_pad a multiple of 64 and rows_out a multiple of the GEMM tile keep the product
 *   on the LDS-DMA GEMM).  The patch embedding is then mafed_gemm(out, W[h, k_pad]^T).
 * mafed_vit_assemble: tokens[b][0] = class_embedding + pos[0], tokens[b][1 + p] = patch_emb[b * np + p] + pos[1 + p] (clip:212-217), fp32.
 * mafed_attn_fwd_bidir: softmax(q k^T D^-0.5) v over all S keys, no mask, no rotary (clip:259-277); qkv [B,S,H,3,D] as in mafed_attn_fwd. */
int mafed_patchify(const void* pixels, mafed_dtype pix_dtype, int B, int C, int H, int W, int patch, int64_t rows_out, int k_pad,
                   void* out, mafed_dtype out_dtype, void* stream);
int mafed_vit_assemble(const void* patch_emb, mafed_dtype pe_dtype, int64_t ld_pe, const float* class_embedding,
                       const float* position_embedding, int B, int num_patches, int h, float* tokens, void* stream);
int mafed_attn_fwd_bidir(const void* qkv, mafed_dtype dtype, int B, int S, int H, int D, void* out, float* lse, void* stream);

/* ---- measurement: per-kernel execution time of the launches this library makes --------------------------------------
 * No reference counterpart (the reference has no profiling); bench.py's `roofline` / `kernels` come from here.
 * Between mafed_prof_begin(max_records) and mafed_prof_end() every hot kernel is launched with a start/stop event pair
 * (hipExtLaunchKernelGGL): the elapsed time of a pair is that dispatch's own execution time on the GPU -- what
 * `rocprofv3 --kernel-trace` reports -- independent of how long the launch sat queued behind other streams.  After the caller
 * has synchronised the device, mafed_prof_collect() returns, in launch order, each record's kernel tag, its algorithmic work
 * (flops for the MFMA kernels, bytes for the HBM-bound ones), its duration in ms and (optionally) its start
 * time in ms relative to the first record's start (host pointers, any may be NULL), and the number of records held.  mafed_prof_tag_name() names a tag.  Launches beyond max_records are not recorded. */
int mafed_prof_begin(int max_records);
int mafed_prof_end(void);
int mafed_prof_collect(int* tags_host, double* work_host, float* ms_host, float* start_ms_host, int max);
const char* mafed_prof_tag_name(int tag);

/* test / tuning hook: 0 = automatic kernel choice, 1 = force the register-staged MFMA GEMM (the ragged-shape kernel),
 * 10 + c = force LDS-DMA tile configuration c; 100 = automatic split-K for accumulate-only outputs, 101 = no split-K,
 * 100 + n = force n K-splits where legal */
int mafed_gemm_set_variant(int variant);
/* 720 = the persistent kernels walk their tiles in the static order (tile = round x grid + slot) whatever the call says, 721 = ticketed
 * order for every multi-round launch (a block's first tile is static, every further one is drawn from a per-XCD queue), 722 = per call
 * (MAFED_EPI_TICKETED; default).
 * mafed_gemm_get_variant reads the hooks back (which = 0: the tile-configuration variant, 7: the persistent-kernel mode 700 / 701 /
 * 710 + c, 72: 720 / 721, 73: launches that ran in ticketed order so far), so that a caller that changes one for a measurement can
 * restore what was set before */
int mafed_gemm_get_variant(int which);
/* 700 = never take the persistent ping-pong kernel, 701 = automatic (default), 710 + c = force its tile configuration c
 * (0: 144x256 tiles, 1: 128x256 tiles, 2: 256x256 tiles) wherever the shape tiles it.  mafed_gemm_pp_launches(): launches that took that kernel so far
 * (tests assert that a forced configuration really ran). */
int mafed_gemm_pp_launches(void);
/* bf16 launches that reached the register-staged MFMA kernel so far: the kernel of last resort, taken when a shape tiles neither the
 * persistent nor the LDS-DMA kernels (K % 64 != 0, or M a multiple of neither 128 nor 144).  Read-only. */
int mafed_gemm_fallback_launches(void);

/* test / tuning hook: 0 = automatic (one-block-per-head "resident" kernels when K/V fit in LDS), 1 = tiled kernels only */
int mafed_attn_set_variant(int variant);

/* test hook: the exact (non-MFMA) forward kernel on bf16 data -- on-GPU cross-check of the MFMA kernels */
int mafed_attn_fwd_exact_bf16(const void* qkv, int B, int S, int H, int D, int rot, const float* rot_cos, const float* rot_sin,
                              const int64_t* attention_mask, int T, void* out, float* lse, void* stream);

/* Tuning helper (not on the product path): occupies `blocks` CUs with one 512-thread block each (`lds_bytes` of LDS) for ~`cycles` shader
 * clocks -- a stand-in for a long-running collective kernel when measuring GEMMs with part of the chip taken (tools/contention_bench.py). */
int mafed_tune_occupy(int blocks, int lds_bytes, long long cycles, void* stream);

/* Tuning helper (not on the product path): `blocks` workgroups of `threads` threads stream `n_bytes` of `src` with 16-byte accesses, `unroll`
 * (2 / 4 / 8) loads in flight per thread; mode 0 reads, 1 copies to dst, 2 = four read + four written streams of n_bytes / 4 (AdamW-shaped).
 * Measures what a FEW CUs stream from HBM while the rest of the chip does something else (tools/stream_cu_bench.py). */
int mafed_tune_stream(const void* src, void* dst, long long n_bytes, int blocks, int threads, int unroll, int mode, void* stream);
/* The AdamW-shaped sweep of mafed_tune_stream, repeated over the buffer for `microseconds` of wall time (100 MHz device clock): a stand-in
 * for the kernels of ONE bucket's all-reduce -- `blocks` = RCCL channels -- on a single GPU (bench.py --emulate-collectives). */
int mafed_tune_stream_for(const void* src, void* dst, long long n_bytes, int blocks, int threads, double microseconds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAFED_HIP_H */
