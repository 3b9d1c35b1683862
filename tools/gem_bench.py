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
import datetime
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 15
dev = "cuda"


def resources():
    """VGPRs, SGPRs, scratch, LDS and occupancy of every kernel in gem.hip as hipcc reports them for gfx950."""
    from mafed_amd import build
    print("# hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage")
    print(f"{'kernel':>36s} {'VGPRs':>6s} {'SGPRs':>6s} {'scratch B/lane':>15s} {'LDS B/block':>12s} {'waves/SIMD':>11s}")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "gem.hip"), "-o",
                            os.path.join(tmp, "o.o")], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    field = lambda block, key: re.search(key + r": (\d+)", block).group(1)
    for block in r.stderr.split("Function Name: ")[1:]:
        name = subprocess.run(["c++filt", block.split()[0]], capture_output=True, text=True).stdout.strip() or block.split()[0]
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("mafed::", "")
        cols = [field(block, key) for key in (" VGPRs", "TotalSGPRs", r"ScratchSize \[bytes/lane\]", r"LDS Size \[bytes/block\]", r"Occupancy \[waves/SIMD\]")]
        print(f"{name:>36s} {cols[0]:>6s} {cols[1]:>6s} {cols[2]:>15s} {cols[3]:>12s} {cols[4]:>11s}")


if "--resources" in sys.argv[1:]:
    resources()
    sys.exit(0)

import torch  # noqa: E402

from mafed_amd import AGEM, GEM, Naive, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402


def timed(fn, reps=REPS, warmup=3):
    """[us per call] from device events around each call."""
    out = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


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
        us = timed(fn)
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

    def samples():
        ids = torch.randint(1, cfg.vocab_size, (n, T), generator=gcpu)
        labels = torch.full((n, T), -100, dtype=torch.int64)
        labels[:, -4:] = ids[:, -4:]
        feats = torch.randn(n, P, cfg.vision_hidden_size, generator=gcpu).to(torch.bfloat16)
        return {"input_ids": ids, "attention_mask": torch.ones(n, T, dtype=torch.int64), "labels": labels, "patch_embeddings": feats}
    first = samples()
    opts = types.SimpleNamespace(tasks=[f"t{i}" for i in range(K + 1)], batch_size=B, seed=1236, pin_mem=False, accumulate_grad_batches=1)
    if method_name == "agem":
        method = AGEM(opts, memory_size=n, model_type="vlpythia")
        method.update(first, model=student)
    elif method_name.startswith("gem"):
        method = GEM(opts, memory_size=n * K, model_type="vlpythia")
        for k in range(K):
            method.update(first if k == 0 else samples(), model=student)
    else:
        method = Naive()
    conf = types.SimpleNamespace(accumulate_grad_batches=1, replay_interval=1, grad_norm=2.0, learning_rate=5e-5, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_perc=0.1)
    tr = Trainer(student, method, conf, task_id=K if method_name != "naive" else 1, n_batches_per_epoch=1000, pipeline_optimizer=True)
    sel = torch.arange(B)
    batch = {k: v[sel].to(dev) for k, v in first.items()}
    batch["max_label_rows"] = 4   # the loader's hint: the row-sparse head (256 of 1024 rows), as the memory batches carry it
    ts, rec = [], None
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        rec = tr.step(dict(batch), i)
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    tr.join()
    torch.cuda.synchronize()
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
    # (``--head SHA``: for a tree that was copied to the GPU box without its .git)
    head = sys.argv[sys.argv.index("--head") + 1] if "--head" in sys.argv[1:] else None
    head = head or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "no git checkout"
    print(f"# python {' '.join(['tools/gem_bench.py'] + sys.argv[1:])}; HEAD {head}; {datetime.datetime.now().isoformat(timespec='seconds')}")
    print(f"# {torch.cuda.get_device_name(0)}; VLPythia-410M bf16 step, B = {B}, {P} + {T} tokens, row-sparse head, pipelined optimiser; wall ms per Trainer.step, "
          "median (min .. max) of 12 after 4")
    n_flat = 0
    for name in ("naive", "agem", "gem1", "gem2", "gem4"):
        n_flat = _step_row(name, cfg, B, P, T)
    print(f"# flat fp32 buffers of {n_flat} elements ({n_flat * 4 / 1e9:.2f} GB each); device-event time around each call, us, median (min .. max) of {REPS}")
    kernel_table(n_flat)
    if "--parent-lib" in sys.argv[1:]:
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent-lib") + 1])
        assert os.path.exists(parent), parent
        print("# naive, the parent commit's library against this tree's, alternating, a fresh process each")
        env0 = {k: v for k, v in os.environ.items() if k not in ("MAFED_HIP_LIB", "MAFED_HIP_LIB_LOOSE")}
        for rnd in (1, 2, 3):
            for who, env in (("parent library", dict(env0, MAFED_HIP_LIB=parent, MAFED_HIP_LIB_LOOSE="1")), ("this tree's library", env0)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--naive-only"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    print(f"## {who}, round {rnd}: the run ended with status {r.returncode}", flush=True)
                    return 1
                print(f"{who + ', round %d' % rnd:>28s}:{r.stdout.strip().split(':', 1)[1]}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
