"""The task-vector merge passes and the step under TaskMerging (run on the GPU box, one process on an otherwise idle
GPU), all in one run:

  * ``merge_fold`` (sum, magmax), the TIES histogram pass alone and the whole TIES fold (7 launches) at density 0.2 over every tensor of
    the VLPythia-410M layout, and ``merge_apply`` (sum / magmax share a kernel; ties) with the bf16 shadow, on flat buffers of the 410M
    parameter count -- beside ``gradnorm_clip``, ``si_stash (task 0)`` and ``mas_penalty``.  Device-event time around each call, median
    and min .. max of REPS calls after a warm-up, and the achieved TB/s against the bytes the call moves.  The yardstick of ``merge_fold``
    is its 16-byte sibling ``si_stash (task 0)``, that of ``merge_apply`` is ``mas_penalty``: the ratio stands beside each row.  The
    whole fold's bytes are 3 x 8 (the histogram passes) + 18 read + 10 written for the share of vectors with a kept element.
  * the 410M bf16 step at B = 32, 256 + 32 tokens with the pipelined optimiser for ``naive``, ``merging`` (TaskMerging after ``begin``;
    nothing is launched inside a step) and ``naive`` again: wall ms around Trainer.step ending in a device synchronise, and beside it the
    free-running figure.
  * with ``--parent-lib PATH``: the ``naive`` step with the parent commit's library (``MAFED_HIP_LIB``) and with this tree's, alternating,
    three rounds, each in a fresh child process.

There is no speed gate: the table is reported as measured.

    python tools/merge_bench.py --parent-lib ../parent/mafed_amd/libmafed_hip.so > profiles/merge.txt
    python tools/merge_bench.py --resources        # no GPU: registers, scratch and LDS of the kernels, from the hipcc gfx950 build
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import parent_lib_ab, resources, run_steps, samples, step_conf, timed, to_dev  # noqa: E402

REPS = 15
FREE_RUNS, FREE_STEPS = 5, 8
DENSITY = 0.2
dev = "cuda"

if "--resources" in sys.argv[1:]:
    resources(("merge.hip",), 44)
    sys.exit(0)

import torch  # noqa: E402

from mafed_amd import Naive, TaskMerging, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402


def kernel_table(n, rows_seg):
    gen = torch.Generator(device=dev).manual_seed(n % 1000003)
    g = torch.randn(n, generator=gen, device=dev) * 1e-3
    base = torch.randn(n, generator=gen, device=dev) * 2e-2
    theta = base + 1e-3 * torch.randn(n, generator=gen, device=dev)
    omega = torch.rand(n, generator=gen, device=dev)
    p, shadow = theta.clone(), theta.to(torch.bfloat16)
    acc, pos, neg = torch.zeros_like(base), torch.zeros_like(base), torch.zeros_like(base)
    counts = torch.zeros(n, 2, dtype=torch.uint8, device=dev)
    sg, sp = torch.empty_like(g), torch.empty_like(g)
    nb = ops.mas_blocks(n)
    sumsq, pen = torch.empty(nb, device=dev), torch.empty(nb, device=dev)
    clip2 = torch.empty(2, device=dev)
    seg = torch.tensor(rows_seg, dtype=torch.int64, device=dev)
    s = seg.size(0)
    blocks = ops.merge_select_blocks(max(m for _, m in rows_seg))
    state, stats = torch.zeros(s, 4, dtype=torch.int64, device=dev), torch.zeros(s, 4, dtype=torch.int64, device=dev)
    hist = torch.zeros(s, ops.PACKNET_BINS, dtype=torch.int32, device=dev)
    drop = 1.0 - DENSITY
    covered = sum(m for _, m in rows_seg)
    stored = 1.0 - drop ** 4                     # the share of vectors with a kept element, if the kept ones lie independently
    for _ in range(2):                          # a state as two earlier tasks leave it, for the apply rows
        ops.merge_ties_fold_(theta, base, pos, neg, counts, seg, blocks, drop, state=state, hist=hist, stats=stats)
        ops.merge_fold_(theta, base, acc, "magmax")
    rows = [
        ("gradnorm_clip", 4, n, None, lambda: ops.gradnorm_clip(g, 2.0, clip2)),
        ("si_stash (task 0)", 16, n, None, lambda: ops.si_stash(g, base, None, None, 0.0, sg, sp, sumsq, pen)),
        ("mas_penalty", 20, n, None, lambda: ops.mas_penalty_(g, base, omega, theta, 1e-6, sumsq, pen)),
        ("merge_fold sum", 16, n, "si_stash (task 0)", lambda: ops.merge_fold_(theta, base, acc, "sum")),
        ("merge_fold magmax", 16, n, "si_stash (task 0)", lambda: ops.merge_fold_(theta, base, acc, "magmax")),
        ("merge_ties_hist pass 0", 8, covered, "gradnorm_clip", lambda: ops.merge_ties_hist(theta, base, seg, blocks, 0, state, hist)),
        (f"ties fold, 7 launches (density {DENSITY})", 24 + 18 + 10 * stored, covered, "si_stash (task 0)",
         lambda: ops.merge_ties_fold_(theta, base, pos, neg, counts, seg, blocks, drop, state=state, hist=hist, stats=stats)),
        ("merge_apply sum / magmax + shadow", 14, n, "mas_penalty", lambda: ops.merge_apply_(p, shadow, base, acc, "magmax", 0.3)),
        ("merge_apply ties + shadow", 20, n, "mas_penalty", lambda: ops.merge_apply_(p, shadow, base, pos, "ties", 0.3, neg=neg, counts=counts)),
    ]
    print(f"{'pass [bytes per parameter]':>48s} {'median us':>10s} {'min':>8s} {'max':>8s} {'MB':>8s} {'TB/s':>6s}   ratio to the sibling")
    rate = {}
    for name, bpp, elems, sibling, fn in rows:
        us = timed(fn, REPS)
        med, nbytes = statistics.median(us), elems * bpp
        rate[name] = nbytes / med / 1e6
        beside = f"   {rate[name] / rate[sibling]:.2f} of {sibling}" if sibling else ""
        print(f"{name + ' [%.3g]' % bpp:>48s} {med:10.1f} {min(us):8.1f} {max(us):8.1f} {nbytes / 1e6:8.1f} {rate[name]:6.2f}{beside}", flush=True)
    st = stats.cpu()
    print(f"# the last TIES fold: {s} tensors, {covered} elements, {int(st[:, 2].sum())} kept ({int(st[:, 2].sum()) / covered:.4f}); "
          f"{blocks} blocks per tensor at most", flush=True)


def step_times(method_name, cfg, B, P, T, steps=12, warmup=4):
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    batch = to_dev(samples(cfg, B, P, T, torch.Generator().manual_seed(1235)), sparse_head=True)
    method = Naive() if method_name == "naive" else TaskMerging(rule="magmax")
    if method_name != "naive":
        method.begin(student)
    tr = Trainer(student, method, step_conf("no_warmup"), task_id=0, n_batches_per_epoch=1000, pipeline_optimizer=True)
    ts, free, rec = run_steps(tr, batch, steps, warmup, free=(FREE_RUNS, FREE_STEPS))
    rows_seg = [[o, m] for o, m, _ in student._offsets.values()]
    return ts, free, float(rec["loss"]), float(rec["grad_norm"]), student.flat_grads.numel(), rows_seg


def _step_row(name, cfg, B, P, T):
    ts, free, loss, gn, n_flat, rows_seg = step_times(name, cfg, B, P, T)
    print(f"{name:>24s}: {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) | {statistics.median(free):7.2f} ({min(free):.2f} .. {max(free):.2f}) ms"
          f"   loss {loss:.4f}  grad norm {gn:.4f}", flush=True)
    torch.cuda.empty_cache()
    return n_flat, rows_seg


def main():
    assert torch.cuda.is_available(), "merge_bench needs a GPU"
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    if "--naive-only" in sys.argv[1:]:
        _step_row("naive", cfg, B, P, T)
        return 0
    print(f"# {torch.cuda.get_device_name(0)}; VLPythia-410M bf16 step, B = {B}, {P} + {T} tokens, row-sparse head, pipelined optimiser; wall ms per Trainer.step, "
          f"median (min .. max): 12 steps after 4, each followed by a synchronise | free-running, {FREE_RUNS} blocks of {FREE_STEPS} steps")
    n_flat, rows_seg = 0, []
    for name in ("naive", "merging", "naive"):
        n_flat, rows_seg = _step_row(name, cfg, B, P, T)
    print(f"# flat buffers of {n_flat} elements ({n_flat * 4 / 1e9:.2f} GB per fp32 buffer); device-event time around each call, us, median (min .. max) of {REPS}")
    kernel_table(n_flat, rows_seg)
    if "--parent-lib" in sys.argv[1:]:
        return parent_lib_ab(__file__, sys.argv[sys.argv.index("--parent-lib") + 1],
                             emit=lambda who, rnd, out: print(f"{who + ', round %d' % rnd:>28s}:{out.strip().split(':', 1)[1]}", flush=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
