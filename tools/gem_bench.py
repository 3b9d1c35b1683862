"""The GEM kernels and step (run on the GPU box, one process on an otherwise idle GPU), all rows from one run:

  * on flat fp32 buffers of the VLPythia-410M parameter count: ``gem_gram`` at K = 1, 2, 4, 8 beside ``agem_dots`` and ``gradnorm_clip``;
    ``gem_project`` at the same K, violated and not, beside ``agem_project``; ``gem_solve`` alone at K = 1 and 8.  Device-event time
    around each call (its streaming kernel plus, where it has one, its one-block finish), median and min .. max of REPS calls after a
    warm-up, and the achieved TB/s against the algorithmic bytes per parameter: gram (K + 1) 4, project (K + 2) 4 (8 when nothing is
    violated: no ref is read), dots 8, agem_project 12 / 8, gradnorm 4.  The buffers are 1.6 GB each, far beyond the 256 MB last-level cache.
  * the 410M bf16 step at B = 32, 256 + 32 tokens, for ``naive``, ``agem`` and ``gem`` with K = 1, 2, 4 finished tasks: wall ms around
    Trainer.step ending in a device synchronise.  GEM runs 1 + K forward + backward per optimiser step by construction.
  * with ``--parent-lib PATH``: the ``naive`` step with the parent commit's library (``MAFED_HIP_LIB``) and with this tree's, alternating,
    three rounds, each in a fresh child process.

There is no speed gate: the table is reported as measured.

    python tools/gem_bench.py --parent-lib ../parent/mafed_amd/libmafed_hip.so [--head SHA] > profiles/gem_step.txt
    python tools/gem_bench.py --resources        # no GPU: registers, scratch and LDS of the kernels, from the hipcc gfx950 build
"""
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import header, parent_lib_ab, resources, run_steps, samples, step_conf, timed, to_dev  # noqa: E402

REPS = 15
dev = "cuda"

if "--resources" in sys.argv[1:]:
    resources(("gem.hip",), 36)
    sys.exit(0)

import torch  # noqa: E402

from mafed_amd import AGEM, GEM, Naive, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402


def kernel_table(n):
    gen = torch.Generator(device=dev).manual_seed(n % 1000003)
    g = torch.randn(n, generator=gen, device=dev) * 1e-3
    refs = [-g + 1e-4 * torch.randn(n, generator=gen, device=dev) for _ in range(8)]   # every constraint violated
    out = torch.empty_like(g)
    clip2 = torch.empty(2, device=dev)
    st4_neg, st4_pos = ops.agem_dots(g, refs[0]).clone(), ops.agem_dots(g, g).clone()
    partials = torch.empty(ops.gem_blocks(n), device=dev)
    stats4 = torch.empty(4, device=dev)
    rows = [("gradnorm_clip", 4, None, lambda: ops.gradnorm_clip(g, 2.0, clip2)),
            ("agem_dots", 8, None, lambda: ops.agem_dots(g, refs[0], stats4))]
    keep = []
    for K in (1, 2, 4, 8):
        gram = ops.gem_gram(g, refs[:K]).clone()
        keep.append(gram)
        rows.append((f"gem_gram K = {K}", 4 * (K + 1), "agem_dots", lambda K=K, gram=gram: ops.gem_gram(g, refs[:K], gram)))
    rows += [("agem_project (violated)", 12, None, lambda: ops.agem_project(g, refs[0], st4_neg, out=out, sumsq_partials=partials)),
             ("agem_project (alpha = 0)", 8, None, lambda: ops.agem_project(g, g, st4_pos, out=out, sumsq_partials=partials))]
    solved = {}
    for K in (1, 2, 4, 8):
        st = ops.gem_solve(ops.gem_gram(g, refs[:K]), K, 0.5, 1e-3).clone()
        st0 = torch.zeros(12, device=dev)
        solved[K] = st
        rows.append((f"gem_project K = {K} (violated)", 4 * (K + 2), "agem_project (violated)",
                     lambda K=K, st=st: ops.gem_project(g, refs[:K], st, out=out, sumsq_partials=partials)))
        rows.append((f"gem_project K = {K} (not violated)", 8, "agem_project (alpha = 0)",
                     lambda K=K, st0=st0: ops.gem_project(g, refs[:K], st0, out=out, sumsq_partials=partials)))
    torch.cuda.synchronize()
    assert float(st4_neg[3]) == 1.0 and float(st4_pos[3]) == 0.0 and all(float(s[8]) == 1.0 for s in solved.values())
    st12 = torch.empty(12, device=dev)
    for K, gram in ((1, keep[0]), (8, keep[3])):
        rows.append((f"gem_solve K = {K}", 0, None, lambda K=K, gram=gram: ops.gem_solve(gram, K, 0.5, 1e-3, st12)))
    rows.append(("stash copy (torch copy_)", 8, None, lambda: out.copy_(g)))
    print(f"{'pass':>34s} {'B/param':>8s} {'median us':>10s} {'min':>8s} {'max':>8s} {'MB':>8s} {'TB/s':>6s}   ratio to the sibling")
    rate = {}
    for name, bpp, sibling, fn in rows:
        us = timed(fn, REPS)
        med = statistics.median(us)
        rate[name] = n * bpp / med / 1e6
        beside = f"   {rate[name] / rate[sibling]:.2f} of {sibling}" if sibling else ""
        print(f"{name:>34s} {bpp:8d} {med:10.1f} {min(us):8.1f} {max(us):8.1f} {n * bpp / 1e6:8.1f} {rate[name]:6.2f}{beside}", flush=True)
    print(f"# gem_solve of the K = 8 Gram above: v {[round(float(x), 4) for x in solved[8][:8]]}, support {int(solved[8][9])}")


def step_times(method_name, cfg, B, P, T, steps=12, warmup=4):
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    gcpu = torch.Generator().manual_seed(1235)
    K = int(method_name[3:]) if method_name.startswith("gem") else 1
    n = 8 * B
    first = samples(cfg, n, P, T, gcpu)
    opts = types.SimpleNamespace(tasks=[f"t{i}" for i in range(K + 1)], batch_size=B, seed=1236, pin_mem=False, accumulate_grad_batches=1)
    if method_name == "agem":
        method = AGEM(opts, memory_size=n, model_type="vlpythia")
        method.update(first, model=student)
    elif method_name.startswith("gem"):
        method = GEM(opts, memory_size=n * K, model_type="vlpythia")
        for k in range(K):
            method.update(first if k == 0 else samples(cfg, n, P, T, gcpu), model=student)   # each task's memory draws on from the one generator
    else:
        method = Naive()
    tr = Trainer(student, method, step_conf("warmup_perc"), task_id=K if method_name != "naive" else 1, n_batches_per_epoch=1000, pipeline_optimizer=True)
    batch = to_dev({k: v[:B] for k, v in first.items()}, sparse_head=True)   # the row-sparse head, as the memory batches carry it
    ts, _, rec = run_steps(tr, batch, steps, warmup)
    parts = ""
    if method_name == "agem":
        parts = f"  (last step: dot {float(method.last_dot):.3e}, alpha {float(method.last_alpha):.3e}, projected {int(method.last_projected)})"
    elif method_name.startswith("gem"):
        parts = (f"  (last step: q {[round(float(x), 3) for x in method.last_gram[0, 1:]]}, v {[round(float(x), 4) for x in method.last_coef[:K]]}, "
                 f"violated {int(method.last_violated)}, support {int(method.last_support)})")
    return ts, rec["branch"], float(rec["loss"]), float(rec["grad_norm"]), parts, student.flat_grads.numel()


def _step_row(name, cfg, B, P, T):
    ts, branch, loss, gn, parts, n_flat = step_times(name, cfg, B, P, T)
    label = name if not name.startswith("gem") else f"gem K = {name[3:]}"
    print(f"{label:>10s} ({branch:>4s} branch): {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) ms   loss {loss:.4f}  grad norm {gn:.4f}{parts}", flush=True)
    torch.cuda.empty_cache()
    return n_flat


def main():
    assert torch.cuda.is_available(), "gem_bench needs a GPU"
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    if "--naive-only" in sys.argv[1:]:
        _step_row("naive", cfg, B, P, T)
        return 0
    print(header(__file__, sys.argv[1:]))
    print(f"# {torch.cuda.get_device_name(0)}; VLPythia-410M bf16 step, B = {B}, {P} + {T} tokens, row-sparse head, pipelined optimiser; wall ms per Trainer.step, "
          "median (min .. max) of 12 after 4")
    n_flat = 0
    for name in ("naive", "agem", "gem1", "gem2", "gem4"):
        n_flat = _step_row(name, cfg, B, P, T)
    print(f"# flat fp32 buffers of {n_flat} elements ({n_flat * 4 / 1e9:.2f} GB each); device-event time around each call, us, median (min .. max) of {REPS}")
    kernel_table(n_flat)
    if "--parent-lib" in sys.argv[1:]:
        return parent_lib_ab(__file__, sys.argv[sys.argv.index("--parent-lib") + 1],
                             emit=lambda who, rnd, out: print(f"{who + ', round %d' % rnd:>28s}:{out.strip().split(':', 1)[1]}", flush=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
