"""The PackNet passes, prune and step (run on the GPU box, one process on an otherwise idle GPU):

  * the 410M bf16 step at B = 32, 256 + 32 tokens with the pipelined optimiser, for ``naive``, ``packnet task 0`` (nothing launched),
    ``packnet task>=1`` (after one prune at 0.5 and update(): half of every layer matrix is trainable, everything else held) and
    ``mas task>=1``.  Wall ms around Trainer.step ending in a device synchronise, and beside it the free-running figure -- blocks of
    steps with one synchronise behind each.  Method names as arguments run only those step rows.
  * a whole ``prune`` over the 410M layout's 96 layer matrices (seven launches, nothing read back), beside the same prune with torch:
    ``kthvalue`` of |p| per tensor on the GPU and masked fills (no float64, no host read either).  Device-event time around the whole call.
  * ``packnet_mask_grad``, ``packnet_hold`` with 0 %, 50 % (independently per element, what a prune leaves) and 100 % held and
    ``packnet_view`` (50 %) on flat buffers of the VLPythia-410M parameter count, beside ``gradnorm_clip``, ``mas_penalty`` and
    ``si_stash (penalty)`` in the same run: device-event time around each call, median and min .. max of REPS calls after a warm-up, and
    the achieved TB/s against the bytes the call moves (a held element: 4 B anchor read, 4 + 2 B written; every element: 1 B owner read).

There is no speed gate: the table is reported as measured.  A per-step pass (mask_grad, hold at 50 % and 100 %) below 0.8 of
``mas_penalty``'s TB/s in the same run is marked.

    python tools/packnet_bench.py > profiles/packnet_step.txt
    python tools/packnet_bench.py --resources        # no GPU: registers and scratch of the kernels, from the hipcc gfx950 build
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import rate_row, resources, run_steps, samples, step_conf, timed, to_dev  # noqa: E402

REPS = 15
FREE_RUNS, FREE_STEPS = 5, 8
dev = "cuda"

if "--resources" in sys.argv[1:]:
    resources(("packnet.hip",), 44)
    sys.exit(0)

import torch  # noqa: E402

from mafed_amd import MAS, Naive, PackNet, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402


def kernel_table(n):
    gen = torch.Generator(device=dev).manual_seed(n % 1000003)
    g = torch.randn(n, generator=gen, device=dev) * 1e-3
    p = torch.randn(n, generator=gen, device=dev) * 2e-2
    anchor = p + 1e-3 * torch.randn(n, generator=gen, device=dev)
    omega = torch.rand(n, generator=gen, device=dev)
    shadow = p.to(torch.bfloat16)
    sg, sp = torch.empty_like(g), torch.empty_like(g)
    half = (torch.rand(n, generator=gen, device=dev) < 0.5).to(torch.uint8)    # owner 1 = trainable in task 1, 0 = held
    ones, zeros = torch.ones(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    held = 1.0 - float(half.float().mean())
    nb = ops.mas_blocks(n)
    sumsq, pen = torch.empty(nb, device=dev), torch.empty(nb, device=dev)
    clip2 = torch.empty(2, device=dev)
    rows = [
        ("gradnorm_clip", 4, lambda: ops.gradnorm_clip(g, 2.0, clip2)),
        ("si_stash (penalty)", 28, lambda: ops.si_stash(g, p, omega, anchor, 1e-6, sg, sp, sumsq, pen)),
        ("mas_penalty", 20, lambda: ops.mas_penalty_(g, p, omega, anchor, 1e-6, sumsq, pen)),
        ("packnet_mask_grad (50 % held)", 9, lambda: ops.packnet_mask_grad_(g, half, 1, sumsq)),
        ("packnet_hold (0 % held)", 1, lambda: ops.packnet_hold_(p, shadow, ones, anchor, 1)),
        ("packnet_hold (50 % held)", 1 + 4 + 6 * held, lambda: ops.packnet_hold_(p, shadow, half, anchor, 1)),
        ("packnet_hold (100 % held)", 11, lambda: ops.packnet_hold_(p, shadow, zeros, anchor, 1)),
        ("packnet_view (50 % zeroed)", 1 + 6 * (1.0 - held), lambda: ops.packnet_view_(p, shadow, half, 0)),
    ]
    print(f"{'pass [bytes per parameter]':>36s} {'median us':>10s} {'min':>8s} {'max':>8s} {'MB':>8s} {'TB/s':>6s}")
    rate = {}
    for name, bpp, fn in rows:
        us = timed(fn, REPS)
        per_step = name.startswith(("packnet_mask_grad", "packnet_hold (50", "packnet_hold (100"))
        below = per_step and n * bpp / statistics.median(us) / 1e6 < 0.8 * rate["mas_penalty"]
        rate[name] = rate_row(f"{name} [{bpp:.3g}]", n * bpp, us, "   <-- below 0.8 of mas_penalty" if below else "")


def prune_times(cfg, reps=7):
    """A whole prune of the 410M model's 96 layer matrices at 0.5, and the same with torch.kthvalue per tensor."""
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    model.sync_shadow()
    pk = PackNet(prune_fraction=0.5)
    pk._ensure(model)
    p0 = model.flat_params.clone()
    names = pk.prunable_names(model)
    elements = sum(model._offsets[name][1] for name in names)

    def reset():
        model.flat_params.copy_(p0)
        pk.owner.zero_()
        pk.pruned = False

    us = timed(lambda: pk.prune(model), reps=reps, warmup=2, before=reset)
    report = pk.prune_report(model)
    exact = all(r["pruned"] >= r["k"] == r["m"] // 2 for r in report.values())
    print(f"{'packnet prune':>36s}: {statistics.median(us) / 1e3:8.2f} ({min(us) / 1e3:.2f} .. {max(us) / 1e3:.2f}) ms   {len(names)} tensors, {elements} elements, "
          f"{sum(r['pruned'] for r in report.values())} pruned, k = m // 2 in every tensor: {exact}", flush=True)
    owner, anchor, shadow = pk.owner, pk.anchor, model.flat_shadow
    views = [(model._offsets[name][0], model._offsets[name][1]) for name in names]

    def torch_prune():
        for o, n in views:
            w = model.flat_params[o:o + n]
            a = w.abs()
            hit = a <= a.kthvalue(n // 2).values
            w.masked_fill_(hit, 0.0)
            anchor[o:o + n].masked_fill_(hit, 0.0)
            shadow[o:o + n].masked_fill_(hit, 0.0)
            owner[o:o + n].masked_fill_(hit, 1)
    try:
        us = timed(torch_prune, reps=reps, warmup=2, before=reset)
        print(f"{'torch kthvalue per tensor':>36s}: {statistics.median(us) / 1e3:8.2f} ({min(us) / 1e3:.2f} .. {max(us) / 1e3:.2f}) ms   "
              f"{int((owner == 1).sum())} pruned", flush=True)
    except Exception as e:   # reported, not hidden: the baseline is torch's, not this project's
        print(f"{'torch kthvalue per tensor':>36s}: failed ({type(e).__name__}: {str(e)[:120]})", flush=True)


def step_times(method_name, cfg, B, P, T, steps=12, warmup=4):
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    dense = to_dev(samples(cfg, B, P, T, torch.Generator().manual_seed(1235)))
    batch = dict(dense, max_label_rows=4)   # the loader's hint: the row-sparse head (256 of 1024 rows)
    method = {"naive": lambda: Naive(), "packnet task 0": lambda: PackNet(), "packnet task>=1": lambda: PackNet(prune_fraction=0.5),
              "mas task>=1": lambda: MAS(reg_lambda=1.0)}[method_name]()
    later = method_name.endswith("task>=1")
    tr = Trainer(student, method, step_conf("no_warmup"), task_id=1 if later else 0, n_batches_per_epoch=1000, pipeline_optimizer=True)
    if later:
        # one step so that the parameters have left their start, then the task boundary (PackNet: prune at 0.5 and consolidate)
        tr.step(dict(batch), 0)
        tr.join()
        method.update(student, dataloader=[dense])
        student.zero_grad()
    ts, free, rec = run_steps(tr, batch, steps, warmup, free=(FREE_RUNS, FREE_STEPS))
    parts = ""
    if isinstance(method, PackNet) and method.owner is not None:
        parts = f"  trainable {float((method.owner == method.task_id).float().mean()):.3f} of the buffer"
    return ts, free, float(rec["loss"]), float(rec["grad_norm"]), parts, student.flat_grads.numel()


def main():
    assert torch.cuda.is_available(), "packnet_bench needs a GPU"
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    print(f"# {torch.cuda.get_device_name(0)}; VLPythia-410M bf16 step, B = {B}, {P} + {T} tokens, row-sparse head, pipelined optimiser; wall ms per Trainer.step, "
          f"median (min .. max): 12 steps after 4, each followed by a synchronise | free-running, {FREE_RUNS} blocks of {FREE_STEPS} steps")
    n_flat = 0
    names = sys.argv[1:] or ["naive", "packnet task 0", "packnet task>=1", "mas task>=1", "naive"]
    for name in names:
        ts, free, loss, gn, parts, n_flat = step_times(name, cfg, B, P, T)
        print(f"{name:>24s}: {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) | {statistics.median(free):7.2f} ({min(free):.2f} .. {max(free):.2f}) ms"
              f"   loss {loss:.4f}  grad norm {gn:.4f}{parts}", flush=True)
        torch.cuda.empty_cache()
    if sys.argv[1:]:
        return
    print("# a whole prune at 0.5 of the same model's layer matrices; device-event time around the call, ms, median (min .. max) of 7 after 2")
    prune_times(cfg)
    torch.cuda.empty_cache()
    print(f"# flat buffers of {n_flat} elements ({n_flat * 4 / 1e9:.2f} GB per fp32 buffer); device-event time around each call, us, median (min .. max) of {REPS}")
    kernel_table(n_flat)


if __name__ == "__main__":
    main()
