"""Shared-image prefill at the headline validation shape (VLPythia-410M, B = 32, 256 image + 32 text tokens, 10 new tokens, bf16; run on
the GPU box): ``generate(image_index=...)`` over N in {32, 16, 8, 4, 1} distinct images, the prompts dealt round-robin to the images,
against the same call on the expanded features without an index (one full prefill per prompt), and the prefill alone for both
(``_prefill``: stack, stores / gather, key rotation and the cache's buffers).  Every time is min / median of the repeats after a warm-up.

    python tools/shared_image_bench.py > profiles/shared_image_decode.txt
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM  # noqa: E402

B, P, T, NEW = 32, 256, 32, 10
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


def main():
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g).to(dev)
    am = torch.ones(B, T, dtype=torch.int64, device=dev)
    images = torch.randn(B, P, cfg.vision_hidden_size, generator=g).to(torch.bfloat16).to(dev)
    print(f"# 410M bf16, B = {B}, {P} + {T} tokens, {NEW} new tokens, prompts dealt round-robin to N images; ms, min / median of {REPS}")
    print(f"# rows through the stack: expanded {B * (P + T)}, shared N * {P} + {B * T}")
    print(f"{'N':>3s} {'rows':>6s}   {'generate, expanded':>20s} {'generate, shared':>20s} {'ratio':>6s}   {'prefill, expanded':>20s} {'prefill, shared':>20s} {'ratio':>6s}")
    for N in (32, 16, 8, 4, 1):
        idx = (torch.arange(B) % N).to(dev)
        feats = images[:N].contiguous()
        expanded = feats.index_select(0, idx)
        kw = dict(input_ids=ids, attention_mask=am, eos_token_id=None, max_new_tokens=NEW)
        ge = wall(lambda: model.generate(patch_embeddings=expanded, **kw))
        gs = wall(lambda: model.generate(patch_embeddings=feats, image_index=idx, **kw))
        pe = wall(lambda: model._prefill(expanded, ids, am, NEW))
        ps = wall(lambda: model._prefill(feats, ids, am, NEW, image_index=idx))
        f = lambda t: f"{t[0]:8.2f} / {t[1]:8.2f}"
        print(f"{N:3d} {N * P + B * T:6d}   {f(ge):>20s} {f(gs):>20s} {gs[1] / ge[1]:6.3f}   {f(pe):>20s} {f(ps):>20s} {ps[1] / pe[1]:6.3f}", flush=True)
    same = model.generate(patch_embeddings=images, input_ids=ids, attention_mask=am, eos_token_id=None, max_new_tokens=NEW)
    shared = model.generate(patch_embeddings=images, image_index=torch.arange(B), input_ids=ids, attention_mask=am, eos_token_id=None, max_new_tokens=NEW)
    print(f"# N = {B}: {int((same == shared).all(dim=1).sum())} of {B} rows pick the same {NEW} tokens on both paths (random weights, bf16)")


if __name__ == "__main__":
    with torch.no_grad():
        main()
