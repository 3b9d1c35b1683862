"""Beam search at the headline validation shape (VLPythia-410M, B = 32, 256 image + 32 text tokens, 10 new tokens, bf16): whole
``generate(num_beams=k)`` and per-step times, cached (shared prefix) and recompute, for k = 1, 3, 5 (run on the GPU box).

    python tools/beam_bench.py                       # one line per k, then the k-beam / greedy step ratios
    rocprofv3 --kernel-trace --stats -d OUT -o beam -- python tools/beam_bench.py --quick   # kernel breakdown of the cached runs
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM  # noqa: E402

B, P, T, NEW = 32, 256, 32, 10
quick = "--quick" in sys.argv
cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
model = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device="cuda", seed=1234)
g = torch.Generator().manual_seed(0)
ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g).cuda()
am = torch.ones(B, T, dtype=torch.int64).cuda()
feats = torch.randn(B, P, cfg.vision_hidden_size, generator=g).to(torch.bfloat16).cuda()


def timed(k, use_cache, new, reps):
    kw = dict(input_ids=ids, attention_mask=am, patch_embeddings=feats, max_new_tokens=new, use_cache=use_cache, eos_token_id=None,
              num_beams=k)
    out = model.generate(**kw)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        out = model.generate(**kw)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


reps = 1 if quick else 5
step = {}
for k in (1, 3, 5):
    t_c, o_c = timed(k, True, NEW, reps)
    t_c1, _ = timed(k, True, 1, reps)            # prefill + first selection only
    step[k] = (t_c - t_c1) / (NEW - 1)
    line = f"k={k}: cached generate {t_c * 1e3:.1f} ms, per step {step[k] * 1e3:.3f} ms"
    if not quick:
        t_u, o_u = timed(k, False, NEW, 2)
        line += f"; recompute generate {t_u * 1e3:.1f} ms ({t_u / t_c:.1f}x), rows equal {float((o_u == o_c).all(1).float().mean()):.2f}"
    print(line, flush=True)
print("step ratio vs greedy: " + ", ".join(f"k={k} {step[k] / step[1]:.2f}x" for k in (3, 5)))
