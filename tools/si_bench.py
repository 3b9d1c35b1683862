"""The Synaptic Intelligence passes and step (run on the GPU box, one process on an otherwise idle GPU):

  * the 410M bf16 step at B = 32, 256 + 32 tokens with the pipelined optimiser, for ``naive``, ``ewc`` (task 1: the penalty through
    autograd) and ``si``: task 0 (stash + path integral) and task >= 1 (plus the penalty gradient).  Wall ms around Trainer.step
    ending in a device synchronise, and beside it the free-running figure -- blocks of steps with one synchronise behind each -- in
    which the pipelined optimiser can run under the next step's forward.  Method names as arguments run only those step rows.
  * ``si_stash`` (both forms), ``si_accumulate`` and ``si_consolidate`` on flat fp32 buffers of the VLPythia-410M parameter count,
    beside ``gradnorm_clip``, ``ewc_penalty_bwd`` and ``agem_project`` in the same run: device-event time around each call, median and
    min .. max of REPS calls after a warm-up, and the achieved TB/s against the algorithmic bytes per parameter.  The buffers are
    1.6 GB each, far beyond the 256 MB last-level cache, so a repeat finds nothing cached.

There is no speed gate: the table is reported as measured.  A pass more than 15 % below the slower of ``ewc_penalty_bwd`` and
``agem_project`` of the same run is marked.

    python tools/si_bench.py > profiles/si_step.txt
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from benchlib import run_steps, samples, step_conf, timed, to_dev  # noqa: E402
from mafed_amd import EWC, SI, Naive, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402

REPS = 15
FREE_RUNS, FREE_STEPS = 5, 8
dev = "cuda"


def kernel_table(n):
    gen = torch.Generator(device=dev).manual_seed(n % 1000003)
    g = torch.randn(n, generator=gen, device=dev) * 1e-3
    p = torch.randn(n, generator=gen, device=dev) * 2e-2
    anchor = p + 1e-3 * torch.randn(n, generator=gen, device=dev)
    omega = torch.rand(n, generator=gen, device=dev)
    w = torch.zeros_like(g)
    sg, sp = torch.empty_like(g), torch.empty_like(g)
    nb = ops.si_blocks(n)
    sumsq, pen = torch.empty(nb, device=dev), torch.empty(nb, device=dev)
    clip2, one = torch.empty(2, device=dev), torch.ones(1, device=dev)
    stats = ops.agem_dots(g, -g).clone()   # violated: the projection reads r and writes g'
    partials = torch.empty(ops.agem_blocks(n), device=dev)
    rows = [
        ("gradnorm_clip", 4, lambda: ops.gradnorm_clip(g, 2.0, clip2)),
        ("ewc_penalty_bwd", 20, lambda: ops.ewc_penalty_bwd_(p, anchor, omega, 1e-6, one, g)),
        ("agem_project (violated)", 12, lambda: ops.agem_project(g, sp, stats, out=sg, sumsq_partials=partials)),
        ("si_stash (task 0)", 16, lambda: ops.si_stash(g, p, None, None, 0.0, sg, sp, sumsq, pen)),
        ("si_stash (penalty)", 28, lambda: ops.si_stash(g, p, omega, anchor, 1e-6, sg, sp, sumsq, pen)),
        ("si_accumulate", 20, lambda: ops.si_accumulate_(sg, anchor, p, w)),
        ("si_consolidate", 28, lambda: ops.si_consolidate_(p, anchor, w, omega, 1e-3)),
    ]
    sp.copy_(g)
    print(f"{'pass':>26s} {'B/param':>8s} {'median us':>10s} {'min':>8s} {'max':>8s} {'MB':>8s} {'TB/s':>6s}")
    rate = {}
    for name, bpp, fn in rows:
        us = timed(fn, REPS)
        med = statistics.median(us)
        rate[name] = n * bpp / med / 1e6
        floor = 0.85 * min(rate.get("ewc_penalty_bwd", 0.0), rate.get("agem_project (violated)", 0.0))
        mark = "   <-- more than 15 % below the slower of ewc_penalty_bwd / agem_project" if name.startswith("si_") and rate[name] < floor else ""
        print(f"{name:>26s} {bpp:8d} {med:10.1f} {min(us):8.1f} {max(us):8.1f} {n * bpp / 1e6:8.1f} {rate[name]:6.2f}{mark}", flush=True)


def step_times(method_name, cfg, B, P, T, steps=12, warmup=4):
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    batch = to_dev(samples(cfg, B, P, T, torch.Generator().manual_seed(1235)), sparse_head=True)
    consolidated = method_name in ("ewc", "si task>=1")
    if method_name == "naive":
        method = Naive()
    elif method_name == "ewc":
        method = EWC(reg_lambda=1.0)
    else:
        method = SI(reg_lambda=1.0)
    tr = Trainer(student, method, step_conf("no_warmup"), task_id=1 if consolidated else 0, n_batches_per_epoch=1000, pipeline_optimizer=True)
    if consolidated:
        # one step so that SI has a path integral to consolidate, then the task boundary
        tr.step(dict(batch), 0)
        tr.join()
        method.update(student, dataloader=[{k: v for k, v in batch.items() if k != "max_label_rows"}])
        student.zero_grad()
    ts, free, rec = run_steps(tr, batch, steps, warmup, free=(FREE_RUNS, FREE_STEPS))
    parts = f"  penalty {float(method.last_penalty):.3e}" if isinstance(method, SI) else ""
    return ts, free, float(rec["loss"]), float(rec["grad_norm"]), parts, student.flat_grads.numel()


def main():
    assert torch.cuda.is_available(), "si_bench needs a GPU"
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    print(f"# {torch.cuda.get_device_name(0)}; VLPythia-410M bf16 step, B = {B}, {P} + {T} tokens, row-sparse head, pipelined optimiser; wall ms per Trainer.step, "
          f"median (min .. max): 12 steps after 4, each followed by a synchronise | free-running, {FREE_RUNS} blocks of {FREE_STEPS} steps")
    n_flat = 0
    names = sys.argv[1:] or ["naive", "ewc", "si task 0", "si task>=1"]
    for name in names:
        ts, free, loss, gn, parts, n_flat = step_times(name, cfg, B, P, T)
        print(f"{name:>24s}: {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) | {statistics.median(free):7.2f} ({min(free):.2f} .. {max(free):.2f}) ms"
              f"   loss {loss:.4f}  grad norm {gn:.4f}{parts}", flush=True)
        torch.cuda.empty_cache()
    if sys.argv[1:]:
        return
    print(f"# flat fp32 buffers of {n_flat} elements ({n_flat * 4 / 1e9:.2f} GB each); device-event time around each call, us, median (min .. max) of {REPS}")
    kernel_table(n_flat)


if __name__ == "__main__":
    main()
