"""Replay-memory selection (run on the GPU box, one process on an otherwise idle GPU):

  * ``ops.select_greedy`` for both modes at (n, d, k) = (20 000, 1024, 1000), (100 000, 1024, 1000) and (100 000, 2048, 1000): device-event
    time around the whole call (2 k + 1 launches, nothing read back), divided by k -- us per pick, median and min .. max of REPS calls
    after a warm-up -- and n d 4 bytes over that time in TB/s, beside ``gradnorm_clip`` over the same n d floats in the same run.
  * the torch formulation of the same loop on the same data: an [n, d] difference, its row sums, the masked arg-best, the host read
    of the winner and the update of v, per pick (TORCH_PICKS picks, us per pick).
  * one ``pooled_features`` forward of VLPythia-410M (bf16, B = 32, 256 + 32 tokens), median of FORWARDS after a warm-up, times the
    n / 32 forwards a selection over n samples needs, and the share of the whole selection that the k picks take next to them.

There is no speed gate: the table is reported as measured.

    python tools/select_bench.py > profiles/memory_selection.txt
    python tools/select_bench.py --resources        # no GPU: registers, LDS and scratch of the kernels, from the hipcc gfx950 build
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import resources, samples, timed, to_dev  # noqa: E402

REPS, TORCH_PICKS, FORWARDS = 5, 50, 12
SHAPES = [(20000, 1024, 1000), (100000, 1024, 1000), (100000, 2048, 1000)]
dev = "cuda"

if "--resources" in sys.argv[1:]:
    # (the scan's template arguments: 16-byte loads, v in LDS, minimise, fold the running minimum; its LDS is dynamic, 16 cdiv(d, 4) + 64 bytes)
    resources(("select.hip",), 56)
    sys.exit(0)

import torch  # noqa: E402

from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402


def torch_greedy(X, mean, mode, k):
    """The same loop in torch, per pick: the [n, d] difference, its row sums, the masked arg-best, the host read, the next v."""
    n = X.shape[0]
    taken = torch.zeros(n, dtype=torch.bool, device=X.device)
    r = mean.clone()
    v = r.float()
    m = torch.full((n,), float("inf"), device=X.device)
    picks = []
    for t in range(k):
        dist = ((X - v) ** 2).sum(dim=1)
        if mode == ops.SELECT_HERDING or t == 0:
            p = int(torch.argmin(dist.masked_fill(taken, float("inf"))))
        else:
            m = torch.minimum(m, dist)
            p = int(torch.argmax(m.masked_fill(taken, float("-inf"))))
        picks.append(p)
        taken[p] = True
        if mode == ops.SELECT_HERDING:
            r = (r + mean) - X[p].double()
            v = r.float()
        else:
            v = X[p]
    return picks


def forward_us():
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    model.sync_shadow()
    b = to_dev(samples(cfg, B, P, T, torch.Generator().manual_seed(1235)))
    out = torch.empty((2, B, cfg.hidden_size), dtype=torch.float32, device=dev)
    us = timed(lambda: model.pooled_features(b["input_ids"], b["attention_mask"], patch_embeddings=b["patch_embeddings"], out=out), FORWARDS)
    del model
    torch.cuda.empty_cache()
    return us


def main():
    assert torch.cuda.is_available(), "select_bench needs a GPU"
    fwd = forward_us()
    fwd_med = statistics.median(fwd)
    print(f"# {torch.cuda.get_device_name(0)}; select_greedy: device-event time around a whole call of k picks / k, median (min .. max) of {REPS} calls after 2;")
    print(f"# torch: the same loop with its per-pick host read, {TORCH_PICKS} picks; gradnorm_clip over the same n d floats in the same run;")
    print(f"# forward: one pooled_features call of VLPythia-410M bf16, B = 32, 256 + 32 tokens, layer -1: {fwd_med / 1e3:.2f} ms "
          f"({min(fwd) / 1e3:.2f} .. {max(fwd) / 1e3:.2f}), median of {FORWARDS} after 3, TIMES the n / 32 forwards of a selection (not run n / 32 times)")
    print(f"{'n':>7s} {'d':>5s} {'k':>5s} {'mode':>8s} {'us/pick':>9s} {'min':>8s} {'max':>8s} {'TB/s':>6s} {'clip TB/s':>10s} {'torch us/pick':>14s} "
          f"{'k picks ms':>11s} {'n/32 fwd ms':>12s} {'picks share':>12s}")
    for n, d, k in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(n + d)
        X = torch.randn(n, d, generator=gen, device=dev)
        mean = ops.cka_stats(X, row_norms=False)[0][0]
        flat, clip2 = X.view(-1), torch.empty(2, device=dev)
        clip = statistics.median(timed(lambda: ops.gradnorm_clip(flat, 2.0, clip2), REPS, warmup=2))
        nbytes = 4.0 * n * d
        for name, mode in (("herding", ops.SELECT_HERDING), ("kcenter", ops.SELECT_KCENTER)):
            us = [t / k for t in timed(lambda: ops.select_greedy(X, mean, mode, k), REPS, warmup=2)]
            med = statistics.median(us)
            tus = [t / TORCH_PICKS for t in timed(lambda: torch_greedy(X, mean, mode, TORCH_PICKS), reps=3, warmup=1)]
            same = torch_greedy(X, mean, mode, 8) == ops.select_greedy(X, mean, mode, 8)[0].tolist()
            picks_ms, fwd_ms = med * k / 1e3, fwd_med * (n / 32) / 1e3
            print(f"{n:7d} {d:5d} {k:5d} {name:>8s} {med:9.1f} {min(us):8.1f} {max(us):8.1f} {nbytes / med / 1e6:6.2f} {nbytes / clip / 1e6:10.2f} "
                  f"{statistics.median(tus):14.1f} {picks_ms:11.1f} {fwd_ms:12.1f} {picks_ms / (picks_ms + fwd_ms):12.3f}"
                  f"{'' if same else '   (first 8 picks differ from torch: a near-tie in fp32)'}", flush=True)
        del X, flat
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
