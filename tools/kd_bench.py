"""The LwF head-loss kernels and step (run on the GPU box, one process on an otherwise idle GPU):

  * ``ce_kd_fwd`` / ``ce_kd_bwd`` against ``ce_fwd`` / ``ce_bwd`` on the same bf16 logits at 1024 x 50304 (the dense head of B = 32, T = 32)
    and 256 x 50304 (its row-sparse head): each kernel's own execution time from the library's profiler (mafed_prof_*: the dispatch's
    begin / end timestamps), median and min .. max of REPS launches after a warm-up, and the achieved TB/s against the algorithmic bytes
    (forward: the logits once -- 1 or 2 matrices; backward: the logits in, the gradient out -- 2 or 3 matrices).  The launches rotate
    over three sets of buffers so that a repeat does not find its operands in the 256 MB last-level cache.
  * the VLPythia-410M step at B = 32, 256 + 32 tokens, bf16, for ``naive``, ``lwf`` and ``featdistill`` (MAFED replay step, the
    configuration bench.py times, on a small replay memory): wall ms around Trainer.step ending in a device synchronise.

The expectation to confirm or refute: each fused pass costs no more than its byte ratio over the cross-entropy kernel it replaces (2x
forward, 1.5x backward) plus the spread between the repeats.  There is no speed gate: the table is reported as measured.

    python tools/kd_bench.py > profiles/lwf_step.txt
"""
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from benchlib import run_steps, samples, step_conf  # noqa: E402
from mafed_amd import CLMethod, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402
from mafed_amd.methods import HBMReplayBuffer  # noqa: E402
from mafed_amd.profiler import KernelProfile  # noqa: E402

V = 50304
REPS = 9
SETS = 3
dev = "cuda"


def kernel_times(rows):
    """{tag: [us per launch]} of the four kernels at [rows, V] bf16 (B = rows / 32 samples of 32 positions, every row but a sample's
    last one labelled: no row is skipped)."""
    B, T = rows // 32, 32
    g = torch.Generator(device=dev).manual_seed(rows)
    sets = []
    for _ in range(SETS):
        s = torch.randn(B, T, V, generator=g, device=dev).to(torch.bfloat16)
        t = (s.float() + 0.1 * torch.randn(B, T, V, generator=g, device=dev)).to(torch.bfloat16)
        sets.append((s, t, torch.empty_like(s)))
    labels = torch.randint(0, V, (B, T), generator=g, device=dev)
    gl = torch.ones(1, device=dev)

    def once(i):
        s, t, d = sets[i % SETS]
        _, lse = ops.ce_fwd(s, labels)
        ops.ce_bwd(s, labels, lse, gl, out=d)
        _, lse3 = ops.ce_kd_fwd(s, t, labels, 2.0, 1.0)
        ops.ce_kd_bwd(s, t, labels, lse3, 2.0, 1.0, gl, out=d)

    for i in range(SETS):
        once(i)
    torch.cuda.synchronize()
    with KernelProfile() as prof:
        for i in range(REPS):
            once(i)
    out = {}
    for tag, work, ms in prof.records():
        if tag in ("ce_fwd", "ce_bwd", "ce_kd_fwd", "ce_kd_bwd"):
            out.setdefault(tag, {"us": [], "bytes": work})["us"].append(ms * 1e3)
    return out


def step_times(method_name, cfg, B, P, T, steps=12, warmup=4):
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    n = 8 * B
    mem = HBMReplayBuffer(B, torch.device(dev), seed=9)
    mem.add(samples(cfg, n, P, T, torch.Generator().manual_seed(1235)))
    opts = types.SimpleNamespace(tasks=["t0", "t1"], batch_size=B, seed=1236, pin_mem=False, accumulate_grad_batches=1)
    gen = torch.Generator(device=dev).manual_seed(1237)
    if method_name == "featdistill":
        method = CLMethod["featdistill"](memory_size=n, opts=opts, model_type="vlpythia", num_hidden_layers=cfg.num_hidden_layers - 1,
                                         distillation_modality_weighing_strategy="balanced", distillation_layer_weighing_strategy="discounted",
                                         gamma=0.5, distillation_layer=None)
        method._update_model(student)
        method.task_id, method.num_vision_tokens, method.mem_dataloader = 1, P, mem
    elif method_name == "lwf":
        method = CLMethod["lwf"](opts=opts, reg_lambda=1.0, temperature=2.0)
        method.update(student)
    else:
        method = CLMethod["naive"]()
    if getattr(method, "past_model", None) is not None:   # the student has moved away from the teacher
        method.past_model.flat_params.add_(torch.randn(method.past_model.flat_params.shape, generator=gen, device=dev) * 1e-3)
        method.past_model._shadow_dirty = True
    tr = Trainer(student, method, step_conf("warmup_perc"), task_id=1, n_batches_per_epoch=1000, pipeline_optimizer=True)
    batch = mem.sample()   # carries the loader's max_label_rows hint: the row-sparse head (256 of 1024 rows)
    ts, _, rec = run_steps(tr, batch, steps, warmup)
    parts = ""
    if method_name == "lwf":
        parts = f"  (last step: CE {float(method.last_ce):.4f}, KD {float(method.last_kd):.3e})"
    return ts, rec["branch"], float(rec["loss"]), parts


def main():
    assert torch.cuda.is_available(), "kd_bench needs a GPU"
    print(f"# {torch.cuda.get_device_name(0)}; bf16 logits [rows, {V}]; kernel time = the dispatch's own execution time, us, median (min .. max) of {REPS}")
    print(f"{'rows':>5s} {'kernel':>10s} {'median us':>10s} {'min':>8s} {'max':>8s} {'MB':>8s} {'TB/s':>6s} {'vs CE kernel':>13s} {'byte ratio':>10s}")
    for rows in (1024, 256):
        tm = kernel_times(rows)
        for tag, base, ratio in (("ce_fwd", None, None), ("ce_kd_fwd", "ce_fwd", 2.0), ("ce_bwd", None, None), ("ce_kd_bwd", "ce_bwd", 1.5)):
            us = tm[tag]["us"]
            med = statistics.median(us)
            rel = f"{med / statistics.median(tm[base]['us']):13.2f} {ratio:10.1f}" if base else f"{'':>13s} {'':>10s}"
            print(f"{rows:5d} {tag:>10s} {med:10.1f} {min(us):8.1f} {max(us):8.1f} {tm[tag]['bytes'] / 1e6:8.1f} {tm[tag]['bytes'] / med / 1e6:6.2f} {rel}", flush=True)
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    print(f"# VLPythia-410M bf16 step, B = {B}, {P} + {T} tokens, row-sparse head, pipelined optimiser; wall ms per Trainer.step, median (min .. max) of 12 after 4")
    for name in ("naive", "lwf", "featdistill"):
        ts, branch, loss, parts = step_times(name, cfg, B, P, T)
        print(f"{name:>12s} ({branch:>6s} branch): {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) ms   loss {loss:.4f}{parts}", flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
