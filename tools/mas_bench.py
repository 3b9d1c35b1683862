"""The Memory Aware Synapses passes, head kernels and step (run on the GPU box, one process on an otherwise idle GPU):

  * the 410M bf16 step at B = 32, 256 + 32 tokens with the pipelined optimiser, for ``naive``, ``ewc`` (task 1: the penalty through
    autograd), ``si task>=1`` and ``mas task>=1``.  Wall ms around Trainer.step ending in a device synchronise, and beside it the
    free-running figure -- blocks of steps with one synchronise behind each.  Method names as arguments run only those step rows.
  * one batch of the importance pass (zero_grad, forward, backward, accumulate; wall ms ending in a synchronise) for MAS -- dense head
    and row-sparse head -- beside one batch of EWC's Fisher pass on the same model.
  * ``mas_accumulate``, ``mas_consolidate`` (both forms) and ``mas_penalty`` on flat fp32 buffers of the VLPythia-410M parameter count,
    beside ``gradnorm_clip``, ``ewc_penalty_bwd`` and ``si_stash (penalty)`` in the same run, and ``sqnorm_fwd`` / ``sqnorm_bwd`` beside
    ``ce_fwd`` / ``ce_bwd`` on bf16 logits of 1024 and 256 rows x 50304 (the dense and the row-sparse head of that batch; every row but
    each sample's last labelled): device-event time around each call, median and min .. max of REPS calls after a warm-up, and the
    achieved TB/s against the bytes the call moves.  The flat buffers are 1.6 GB each, far beyond the 256 MB last-level cache; the logits
    are 103 / 26 MB and may be found there, for the cross-entropy rows as for the squared-norm ones.

There is no speed gate: the table is reported as measured.  ``mas_penalty`` more than 10 % below ``ewc_penalty_bwd`` (the same 20 B per
parameter) of the same run is marked.

    python tools/mas_bench.py > profiles/mas_step.txt
    python tools/mas_bench.py --resources        # no GPU: registers and scratch of the kernels, from the hipcc gfx950 build
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import rate_row, resources, run_steps, samples, step_conf, timed, to_dev  # noqa: E402

REPS = 15
FREE_RUNS, FREE_STEPS = 5, 8
dev = "cuda"

if "--resources" in sys.argv[1:]:
    resources(("mas.hip", "sqnorm.hip", "si.hip"), 58, lds=False)
    sys.exit(0)

import torch  # noqa: E402

from mafed_amd import EWC, MAS, SI, Naive, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402


def kernel_table(n):
    gen = torch.Generator(device=dev).manual_seed(n % 1000003)
    g = torch.randn(n, generator=gen, device=dev) * 1e-3
    p = torch.randn(n, generator=gen, device=dev) * 2e-2
    anchor = p + 1e-3 * torch.randn(n, generator=gen, device=dev)
    omega = torch.rand(n, generator=gen, device=dev)
    acc = torch.zeros_like(g)
    sg, sp = torch.empty_like(g), torch.empty_like(g)
    nb = ops.mas_blocks(n)
    sumsq, pen = torch.empty(nb, device=dev), torch.empty(nb, device=dev)
    clip2, one = torch.empty(2, device=dev), torch.ones(1, device=dev)
    rows = [
        ("gradnorm_clip", 4, lambda: ops.gradnorm_clip(g, 2.0, clip2)),
        ("ewc_penalty_bwd", 20, lambda: ops.ewc_penalty_bwd_(p, anchor, omega, 1e-6, one, g)),
        ("si_stash (penalty)", 28, lambda: ops.si_stash(g, p, omega, anchor, 1e-6, sg, sp, sumsq, pen)),
        ("mas_penalty", 20, lambda: ops.mas_penalty_(g, p, omega, anchor, 1e-6, sumsq, pen)),
        ("mas_accumulate", 12, lambda: ops.mas_accumulate_(g, acc, 32.0)),
        ("mas_consolidate (first)", 20, lambda: ops.mas_consolidate_(acc, omega, p, sp, 1.0 / 32, 0.5, True)),
        ("mas_consolidate (later)", 24, lambda: ops.mas_consolidate_(acc, omega, p, sp, 1.0 / 32, 0.5, False)),
    ]
    print(f"{'pass [bytes per parameter]':>36s} {'median us':>10s} {'min':>8s} {'max':>8s} {'MB':>8s} {'TB/s':>6s}")
    rate = {}
    for name, bpp, fn in rows:
        us = timed(fn, REPS)
        below = name == "mas_penalty" and n * bpp / statistics.median(us) / 1e6 < 0.9 * rate["ewc_penalty_bwd"]
        rate[name] = rate_row(f"{name} [{bpp}]", n * bpp, us, "   <-- more than 10 % below ewc_penalty_bwd" if below else "")
    del g, p, anchor, omega, acc, sg, sp
    torch.cuda.empty_cache()
    V = 50304
    for B, T in ((32, 32), (32, 8)):
        R = B * T
        z = torch.randn(B, T, V, generator=gen, device=dev).to(torch.bfloat16)
        lab = torch.randint(0, V, (B, T), generator=gen, device=dev)
        labelled = B * (T - 1)
        out = torch.empty_like(z)
        _, lse = ops.ce_fwd(z, lab)
        for name, nbytes, fn in (
                (f"ce_fwd {R} x {V}", R * V * 2, lambda: ops.ce_fwd(z, lab)),
                (f"sqnorm_fwd {R} x {V}", labelled * V * 2, lambda: ops.sqnorm_fwd(z, lab)),
                (f"ce_bwd {R} x {V}", (labelled + R) * V * 2, lambda: ops.ce_bwd(z, lab, lse, one, out=out)),
                (f"sqnorm_bwd {R} x {V}", (labelled + R) * V * 2, lambda: ops.sqnorm_bwd(z, lab, one, out=out))):
            rate_row(name, nbytes, timed(fn, REPS))
        del z, out


def _batch(cfg, B, P, T):
    return to_dev(samples(cfg, B, P, T, torch.Generator().manual_seed(1235)))


def step_times(method_name, cfg, B, P, T, steps=12, warmup=4):
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    dense = _batch(cfg, B, P, T)
    batch = dict(dense, max_label_rows=4)   # the loader's hint: the row-sparse head (256 of 1024 rows)
    method ={"naive": Naive, "ewc": EWC, "si task>=1": SI, "mas task>=1": MAS}[method_name](**({} if method_name == "naive" else {"reg_lambda": 1.0}))
    consolidated = method_name != "naive"
    tr = Trainer(student, method, step_conf("no_warmup"), task_id=1 if consolidated else 0, n_batches_per_epoch=1000, pipeline_optimizer=True)
    if consolidated:
        # one step so that the parameters have left their start (and SI has a path integral to consolidate), then the task boundary
        tr.step(dict(batch), 0)
        tr.join()
        method.update(student, dataloader=[dense])
        student.zero_grad()
    ts, free, rec = run_steps(tr, batch, steps, warmup, free=(FREE_RUNS, FREE_STEPS))
    parts = f"  penalty {float(method.last_penalty):.3e}" if isinstance(method, (SI, MAS)) else ""
    return ts, free, float(rec["loss"]), float(rec["grad_norm"]), parts, student.flat_grads.numel()


def importance_times(cfg, B, P, T, reps=7):
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    dense = _batch(cfg, B, P, T)
    sparse = dict(dense, max_label_rows=4)
    mas, ewc = MAS(), EWC(reg_lambda=1.0)
    for name, fn in (("ewc fisher batch (dense head)", lambda: ewc.compute_importances(student, [dense])),
                     ("mas importance batch (dense head)", lambda: mas.compute_importances(student, [dense])),
                     ("mas importance batch (row-sparse head)", lambda: mas.compute_importances(student, [sparse]))):
        ts = []
        for k in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        print(f"{name:>40s}: {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) ms", flush=True)


def main():
    assert torch.cuda.is_available(), "mas_bench needs a GPU"
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    print(f"# {torch.cuda.get_device_name(0)}; VLPythia-410M bf16 step, B = {B}, {P} + {T} tokens, row-sparse head, pipelined optimiser; wall ms per Trainer.step, "
          f"median (min .. max): 12 steps after 4, each followed by a synchronise | free-running, {FREE_RUNS} blocks of {FREE_STEPS} steps")
    n_flat = 0
    names = sys.argv[1:] or ["naive", "ewc", "si task>=1", "mas task>=1"]
    for name in names:
        ts, free, loss, gn, parts, n_flat = step_times(name, cfg, B, P, T)
        print(f"{name:>24s}: {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) | {statistics.median(free):7.2f} ({min(free):.2f} .. {max(free):.2f}) ms"
              f"   loss {loss:.4f}  grad norm {gn:.4f}{parts}", flush=True)
        torch.cuda.empty_cache()
    if sys.argv[1:]:
        return
    print(f"# one batch of the importance pass on the same model and batch: zero_grad, forward, backward, accumulate (the scaling pass behind it included); wall ms, "
          f"median (min .. max) of 7 after 2")
    importance_times(cfg, B, P, T)
    torch.cuda.empty_cache()
    print(f"# flat fp32 buffers of {n_flat} elements ({n_flat * 4 / 1e9:.2f} GB each) and bf16 logits; device-event time around each call, us, median (min .. max) of {REPS}")
    kernel_table(n_flat)


if __name__ == "__main__":
    main()
