"""The A-GEM projection kernels and step (run on the GPU box, one process on an otherwise idle GPU):

  * ``agem_dots`` and ``agem_project`` on flat fp32 buffers of the VLPythia-410M parameter count, beside the project's other flat-buffer
    passes ``gradnorm_clip`` and ``ewc_penalty_fwd`` in the same run: device-event time around each call (its streaming kernel plus,
    where it has one, its one-block finish), median and min .. max of REPS calls after a warm-up, and the achieved TB/s against the
    algorithmic bytes per parameter (gradnorm 4, dots 8, project 12 -- g and r in, g' out --, ewc 12).  The buffers are 1.6 GB each, far
    beyond the 256 MB last-level cache, so a repeat finds nothing cached.  ``project`` is timed on both branches: a violated constraint
    (r = -g + noise) and alpha = 0 (r = g), which copies g without reading r (8 bytes per parameter).
  * the 410M bf16 step at B = 32, 256 + 32 tokens, for ``naive`` against ``agem`` with a filled memory: wall ms around Trainer.step
    ending in a device synchronise.  A-GEM runs a second forward + backward on a memory batch in every optimiser step, so its step is
    roughly two of Naive's by construction; the projection itself is the two passes above plus the stash copy.

There is no speed gate: the table is reported as measured.

    python tools/agem_bench.py > profiles/agem_step.txt
"""
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from benchlib import run_steps, samples, step_conf, timed, to_dev  # noqa: E402
from mafed_amd import AGEM, Naive, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402

REPS = 15
dev = "cuda"


def kernel_table(n):
    gen = torch.Generator(device=dev).manual_seed(n % 1000003)
    g = torch.randn(n, generator=gen, device=dev) * 1e-3
    r_neg = -g + 1e-4 * torch.randn(n, generator=gen, device=dev)
    r_pos = g.clone()
    out = torch.empty_like(g)
    clip2 = torch.empty(2, device=dev)
    pen = torch.zeros(1, device=dev)
    st_neg, st_pos = ops.agem_dots(g, r_neg).clone(), ops.agem_dots(g, r_pos).clone()
    partials = torch.empty(ops.agem_blocks(n), device=dev)
    torch.cuda.synchronize()
    assert float(st_neg[3]) == 1.0 and float(st_pos[3]) == 0.0
    stats = torch.empty(4, device=dev)
    rows = [
        ("gradnorm_clip", 4, lambda: ops.gradnorm_clip(g, 2.0, clip2)),
        ("ewc_penalty_fwd", 12, lambda: ops.ewc_penalty_fwd(g, r_neg, r_pos, 0.5, out=pen)),
        ("agem_dots", 8, lambda: ops.agem_dots(g, r_neg, stats)),
        ("agem_project (violated)", 12, lambda: ops.agem_project(g, r_neg, st_neg, out=out, sumsq_partials=partials)),
        ("agem_project (alpha = 0)", 8, lambda: ops.agem_project(g, r_pos, st_pos, out=out, sumsq_partials=partials)),
        ("stash copy (torch copy_)", 8, lambda: out.copy_(g)),
    ]
    print(f"{'pass':>26s} {'B/param':>8s} {'median us':>10s} {'min':>8s} {'max':>8s} {'MB':>8s} {'TB/s':>6s}")
    for name, bpp, fn in rows:
        us = timed(fn, REPS)
        med = statistics.median(us)
        print(f"{name:>26s} {bpp:8d} {med:10.1f} {min(us):8.1f} {max(us):8.1f} {n * bpp / 1e6:8.1f} {n * bpp / med / 1e6:6.2f}", flush=True)


def step_times(method_name, cfg, B, P, T, steps=12, warmup=4):
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    n = 8 * B
    mem = samples(cfg, n, P, T, torch.Generator().manual_seed(1235))
    opts = types.SimpleNamespace(tasks=["t0", "t1"], batch_size=B, seed=1236, pin_mem=False, accumulate_grad_batches=1)
    if method_name == "agem":
        method = AGEM(opts, memory_size=n, model_type="vlpythia")
        method.update(mem, model=student)
    else:
        method = Naive()
    tr = Trainer(student, method, step_conf("warmup_perc"), task_id=1, n_batches_per_epoch=1000, pipeline_optimizer=True)
    batch = to_dev({k: v[:B] for k, v in mem.items()}, sparse_head=True)   # the row-sparse head, as the memory batches carry it
    ts, _, rec = run_steps(tr, batch, steps, warmup)
    parts = ""
    if method_name == "agem":
        parts = (f"  (last step: dot {float(method.last_dot):.3e}, rsq {float(method.last_ref_sq):.3e}, alpha {float(method.last_alpha):.3e}, "
                 f"projected {int(method.last_projected)})")
    n_flat = student.flat_grads.numel()
    return ts, rec["branch"], float(rec["loss"]), float(rec["grad_norm"]), parts, n_flat


def main():
    assert torch.cuda.is_available(), "agem_bench needs a GPU"
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    print(f"# {torch.cuda.get_device_name(0)}; VLPythia-410M bf16 step, B = {B}, {P} + {T} tokens, row-sparse head, pipelined optimiser; wall ms per Trainer.step, "
          "median (min .. max) of 12 after 4")
    n_flat = 0
    for name in ("naive", "agem"):
        ts, branch, loss, gn, parts, n_flat = step_times(name, cfg, B, P, T)
        print(f"{name:>8s} ({branch:>4s} branch): {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) ms   loss {loss:.4f}  grad norm {gn:.4f}{parts}", flush=True)
        torch.cuda.empty_cache()
    print(f"# flat fp32 buffers of {n_flat} elements ({n_flat * 4 / 1e9:.2f} GB each); device-event time around each call, us, median (min .. max) of {REPS}")
    kernel_table(n_flat)


if __name__ == "__main__":
    main()
