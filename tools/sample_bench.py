"""Sampled decoding at the headline validation shape (VLPythia-410M, B = 32, 256 image + 32 text tokens, 10 new tokens, bf16; run on
the GPU box): ``model.sample`` at n = 1 (eager and replayed from the hipGraph) and n = 3 / 5 over the shared prefix, beside
``generate`` greedy and beam search at k = 3 / 5 from the same process; then the sampler kernel alone (``mafed_sample_token``, V =
50 304, R = 32 / 96 / 160) as a hipGraph chain of back-to-back launches, beside ``mafed_beam_candidates`` and a torch restatement of the
same pick (softmax, sort, cumsum, masks, multinomial) on the same logits.  Every time is min / median of the repeats after a warm-up.

    python tools/sample_bench.py > profiles/sample_decode.txt
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402

B, P, T, NEW, V = 32, 256, 32, 10, 50304
WARP = dict(temperature=0.8, top_k=50, top_p=0.95, min_p=0.0)
REPS, CHAIN = 7, 20
dev = "cuda"


def mm(ts):
    return min(ts), statistics.median(ts)


def wall(fn, reps=REPS):
    """min / median wall seconds of fn() ending in a device synchronise, after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return mm(ts)


def end_to_end():
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g).to(dev)
    am = torch.ones(B, T, dtype=torch.int64, device=dev)
    feats = torch.randn(B, P, cfg.vision_hidden_size, generator=g).to(torch.bfloat16).to(dev)
    kw = dict(input_ids=ids, attention_mask=am, patch_embeddings=feats, eos_token_id=None)
    runs = {
        "generate greedy, eager": lambda new, **x: model.generate(max_new_tokens=new, **kw, **x),
        "generate greedy, graph": lambda new, **x: model.generate(max_new_tokens=new, use_graph=True, **kw, **x),
        "sample n=1, eager": lambda new, **x: model.sample(max_new_tokens=new, seed=7, **WARP, **kw, **x),
        "sample n=1, graph": lambda new, **x: model.sample(max_new_tokens=new, seed=7, use_graph=True, **WARP, **kw, **x),
        "generate beam k=3": lambda new, **x: model.generate(max_new_tokens=new, num_beams=3, **kw, **x),
        "sample n=3, shared prefix": lambda new, **x: model.sample(max_new_tokens=new, seed=7, num_return_sequences=3, **WARP, **kw, **x),
        "generate beam k=5": lambda new, **x: model.generate(max_new_tokens=new, num_beams=5, **kw, **x),
        "sample n=5, shared prefix": lambda new, **x: model.sample(max_new_tokens=new, seed=7, num_return_sequences=5, **WARP, **kw, **x),
    }
    print(f"# end to end: 410M bf16, B = {B}, {P} + {T} tokens, {NEW} new tokens; per step = (t({NEW} tokens) - t(1 token)) / {NEW - 1}, min / median of {REPS}")
    step = {}
    for name, fn in runs.items():
        full = wall(lambda: fn(NEW))
        one = wall(lambda: fn(1))   # prefill + the first pick (a graph run of one token is the eager path)
        step[name] = tuple((f - o) / (NEW - 1) for f, o in zip(full, one))
        print(f"{name:28s} whole call {full[0] * 1e3:7.2f} / {full[1] * 1e3:7.2f} ms   per step {step[name][0] * 1e3:6.3f} / {step[name][1] * 1e3:6.3f} ms", flush=True)
    a, b = step["sample n=1, eager"][1], step["generate greedy, eager"][1]
    print(f"sampled step - greedy step (eager, medians): {(a - b) * 1e6:+.1f} us;  graph: "
          f"{(step['sample n=1, graph'][1] - step['generate greedy, graph'][1]) * 1e6:+.1f} us")
    for n in (3, 5):
        print(f"n = {n} sampled step / k = {n} beam step (medians): {step[f'sample n={n}, shared prefix'][1] / step[f'generate beam k={n}'][1]:.3f}")
    del model
    torch.cuda.empty_cache()


def chain(body, per=CHAIN, reps=REPS):
    """min / median microseconds per launch of ``body`` (``per`` launches) replayed from a hipGraph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        body()
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); gr.replay(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / per)
    return mm(ts)


def torch_pick(logits, temperature, top_k, top_p, min_p):
    """The same pick as HF runs it: warpers on a sorted copy, softmax, multinomial."""
    s = logits.float() / temperature
    if top_k > 0:
        s = s.masked_fill(s < torch.topk(s, top_k)[0][..., -1, None], -float("inf"))
    if top_p < 1.0:
        sl, si = torch.sort(s, descending=False)
        remove = sl.softmax(-1).cumsum(-1) <= 1 - top_p
        remove[..., -1:] = False
        s = s.masked_fill(remove.scatter(1, si, remove), -float("inf"))
    if min_p > 0.0:
        pr = s.softmax(-1)
        s = s.masked_fill(pr < min_p * pr.max(-1, keepdim=True)[0], -float("inf"))
    return torch.multinomial(s.softmax(-1), 1).squeeze(1)


def kernel_alone():
    print(f"\n# the pick alone, V = {V}, bf16 logits: us per launch, min / median of {REPS} replays of a {CHAIN}-launch hipGraph chain"
          " (torch restatement: eager launches between two events, it cannot be captured)")
    g = torch.Generator().manual_seed(1)
    sets = [("T 1", (1.0, 0, 1.0, 0.0)), ("T 0.8, k 50, p 0.95", (0.8, 50, 0.95, 0.0)), ("T 1.3, p 0.9", (1.3, 0, 0.9, 0.0)),
            ("min_p 0.05", (1.0, 0, 1.0, 0.05)), ("T 1.5, k 20, p 0.8, min_p 0.02", (1.5, 20, 0.8, 0.02))]
    x = torch.zeros(64, device=dev)
    floor = chain(lambda: [x.add_(1.0) for _ in range(CHAIN)])
    print(f"{'(a 64-element add_: the floor of a launch in a chain)':64s} {floor[0]:7.2f} / {floor[1]:7.2f}")
    for R in (32, 96, 160):
        logits = (2.0 * torch.randn(R, V, generator=g)).to(torch.bfloat16).to(dev)
        seed = ops.seed_word(11, dev)
        tok = torch.empty(R, dtype=torch.int64, device=dev)
        lp = torch.empty(R, dtype=torch.float32, device=dev)
        for name, w in sets:
            t = chain(lambda: [ops.sample_token(logits, *w, seed=seed, step=i, token=tok, logprob=lp) for i in range(CHAIN)])
            print(f"{'mafed_sample_token R = %3d, %s' % (R, name):64s} {t[0]:7.2f} / {t[1]:7.2f}   ({R * V * 2 / t[0] / 1e6:.2f} TB/s of logits)", flush=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for name, w in sets[:3]:
            for _ in range(3):
                torch_pick(logits, *w)
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPS):
                e0.record(); torch_pick(logits, *w); e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            print(f"{'torch restatement    R = %3d, %s' % (R, name):64s} {min(ts):7.2f} / {statistics.median(ts):7.2f}", flush=True)
        if R % 32 == 0 and R // 32 in (1, 3, 5):
            k = R // 32
            score = torch.zeros(R, dtype=torch.float32, device=dev)
            out = ops.beam_candidates(logits, score, 32, k)
            t = chain(lambda: [ops.beam_candidates(logits, score, 32, k, out=out) for _ in range(CHAIN)])
            print(f"{'mafed_beam_candidates B = 32, k = %d (the same %d rows)' % (k, R):64s} {t[0]:7.2f} / {t[1]:7.2f}", flush=True)


if __name__ == "__main__":
    if "--kernel-only" not in sys.argv:
        end_to_end()
    kernel_alone()
