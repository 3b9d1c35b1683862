"""``model.score`` at the headline validation shape (VLPythia-410M, B = 32, 256 image + 32 text tokens, A = 6 answer tokens, bf16; run on the
GPU box): C in {1, 2, 4, 8, 16} candidates per prompt on the shared path (one prefill per prompt, the candidate rows behind it) against
the expanded path (``use_cache=False``: the B * C sequences through the engine forward), the rows each moves through the stack, the
launches per call that reached the register-staged GEMM (``mafed_gemm_fallback_launches``), and ``ops.attn_cand_fwd`` alone on one
layer's shapes.  Every time is min / median of the repeats after a warm-up.  There is no speed gate: the table is reported as measured.

    python tools/score_bench.py > profiles/score.txt
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM, _lib, ops  # noqa: E402

B, P, T, A = 32, 256, 32, 6
REPS = 7
dev = "cuda"


def wall(fn, reps=REPS):
    """min / median wall milliseconds of fn() ending in a device synchronise, after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), statistics.median(ts)


def fallbacks(fn):
    lib = _lib.load()
    n0 = lib.mafed_gemm_fallback_launches()
    fn()
    torch.cuda.synchronize()
    return lib.mafed_gemm_fallback_launches() - n0


def main():
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    H, D, S0 = cfg.num_attention_heads, cfg.head_dim, P + T
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g).to(dev)
    am = torch.ones(B, T, dtype=torch.int64, device=dev)
    feats = torch.randn(B, P, cfg.vision_hidden_size, generator=g).to(torch.bfloat16).to(dev)
    f = lambda t: f"{t[0]:8.2f} / {t[1]:8.2f}"
    print(f"# 410M bf16, B = {B}, {P} + {T} tokens, A = {A} answer tokens, C candidates per prompt; ms, min / median of {REPS}")
    print(f"# rows through the stack: expanded B * C * {S0 + A}, shared B * {S0} + B * C * A_run")
    print(f"{'C':>3s} {'A_run':>5s} {'rows exp':>9s} {'rows shared':>11s}   {'score, expanded':>20s} {'score, shared':>20s} {'ratio':>6s}   "
          f"{'fallback exp':>12s} {'fallback shared':>15s}   {'attn_cand_fwd alone':>20s}")
    for C in (1, 2, 4, 8, 16):
        cand = torch.randint(1, cfg.vocab_size, (B, C, A), generator=g).to(dev)
        kw = dict(input_ids=ids, attention_mask=am, patch_embeddings=feats, candidate_ids=cand)
        A_run = model.padded_candidate_len(B * C, A)
        se = wall(lambda: model.score(use_cache=False, **kw))
        ss = wall(lambda: model.score(use_cache=True, **kw))
        fe, fs = fallbacks(lambda: model.score(use_cache=False, **kw)), fallbacks(lambda: model.score(use_cache=True, **kw))
        pre = torch.randn(B * S0, 3 * H * D, generator=g).to(torch.bfloat16).to(dev)
        qc = torch.randn(B * C * A_run, 3 * H * D, generator=g).to(torch.bfloat16).to(dev)
        cos, sin = model.rotary_tables(S0 + A_run)
        ka = wall(lambda: ops.attn_cand_fwd(pre, S0, qc, C, A_run, B, H, D, cfg.rotary_ndims, cos, sin, am))
        print(f"{C:3d} {A_run:5d} {B * C * (S0 + A):9d} {B * S0 + B * C * A_run:11d}   {f(se):>20s} {f(ss):>20s} {ss[1] / se[1]:6.3f}   "
              f"{fe:12d} {fs:15d}   {f(ka):>20s}", flush=True)
    C = 8
    cand = torch.randint(1, cfg.vocab_size, (B, C, A), generator=g).to(dev)
    kw = dict(input_ids=ids, attention_mask=am, patch_embeddings=feats, candidate_ids=cand, return_token_logprobs=True)
    (s_e, t_e), (s_s, t_s) = model.score(use_cache=False, **kw), model.score(use_cache=True, **kw)
    print(f"# C = {C}: max |token log-probability, shared - expanded| {float((t_s - t_e).abs().max()):.3e} at max |log-probability| "
          f"{float(t_e.abs().max()):.2f}; {int((s_s.argmax(-1) == s_e.argmax(-1)).sum())} of {B} prompts rank the same candidate first "
          "(random weights, bf16)")


if __name__ == "__main__":
    with torch.no_grad():
        main()
