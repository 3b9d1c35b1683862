"""The DER++ head-loss kernels, recording pass and step (run on the GPU box, one process on an otherwise idle GPU):

  * ``ce_mse_fwd`` / ``ce_mse_bwd`` beside ``ce_fwd`` / ``ce_bwd`` and ``ce_kd_fwd`` / ``ce_kd_bwd`` on the same bf16 logits at
    1024 x 50304 (the dense head of B = 32, T = 32) and 256 x 50304 (its row-sparse head): each kernel's own execution time from the
    library's profiler (mafed_prof_*: the dispatch's begin / end timestamps), median and min .. max of REPS launches after a warm-up, and
    the achieved TB/s against the algorithmic bytes (forward: the logits once -- 1 or 2 matrices; backward: the logits in, the gradient
    out -- 2 or 3 matrices).  The store is [4000, 4, 50304] bf16 (1.6 GB), ``mem_index`` random.  A sample has four positions, the
    first three labelled (a stored row exists for at most four): every kernel skips a sample's last row, so the MB and TB/s columns,
    which count whole matrices, overstate what was moved by up to a quarter -- for all six alike.  The launches rotate over three sets
    of logits.
  * the VLPythia-410M step at B = 32, 256 + 32 tokens, bf16, pipelined optimiser, for ``naive``, ``replay`` (ER) and ``der``, the last
    two with every step a replay step over a 256-sample memory: wall ms around Trainer.step ending in a device synchronise.
  * one recording pass (``DER.update`` less ``ER.update``: ``model.answer_logits`` in batches of 32) over 1000 samples.
  * with ``--parent-lib PATH``: the ``naive`` step with the parent commit's library (``MAFED_HIP_LIB``) and with this tree's,
    alternating, three rounds, each in a fresh child process.

The expectations to confirm or refute: the ce_mse pair moves the bytes of the ce_kd pair with less arithmetic and should take no longer;
the ``der`` replay step should cost what ``replay`` does plus the difference of the head kernels.  There is no speed gate: the table is
reported as measured.

    python tools/der_bench.py --parent-lib ../parent/mafed_amd/libmafed_hip.so [--head SHA] > profiles/der_step.txt
    python tools/der_bench.py --resources        # no GPU: registers, scratch and LDS of the kernels, from the hipcc gfx950 build
"""
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import header, parent_lib_ab, resources, run_steps, samples, step_conf, to_dev  # noqa: E402

V = 50304
REPS = 9
SETS = 3
N_MEM, A = 4000, 4
dev = "cuda"

if "--resources" in sys.argv[1:]:
    resources(("der.hip", "ce.hip", "kd.hip"), 52, renames=(("unsigned short", "bf16"),))   # der.hip beside the kernels it is measured against
    sys.exit(0)

import torch  # noqa: E402

from mafed_amd import CLMethod, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops  # noqa: E402
from mafed_amd.profiler import KernelProfile  # noqa: E402

TAGS = ("ce_fwd", "ce_bwd", "ce_kd_fwd", "ce_kd_bwd", "ce_mse_fwd", "ce_mse_bwd")


def kernel_times(rows, store):
    """{tag: [us per launch]} of the six kernels at [rows, V] bf16: B = rows / 4 samples of 4 positions, every row but a sample's last
    one labelled."""
    T = 4
    B = rows // T
    g = torch.Generator(device=dev).manual_seed(rows)
    sets = []
    for _ in range(SETS):
        s = torch.randn(B, T, V, generator=g, device=dev).to(torch.bfloat16)
        t = (s.float() + 0.1 * torch.randn(B, T, V, generator=g, device=dev)).to(torch.bfloat16)
        sets.append((s, t, torch.empty_like(s)))
    labels = torch.randint(0, V, (B, T), generator=g, device=dev)
    mi = torch.randint(0, N_MEM, (B,), generator=g, device=dev)
    gl = torch.ones(1, device=dev)

    def once(i):
        s, t, d = sets[i % SETS]
        _, lse = ops.ce_fwd(s, labels)
        ops.ce_bwd(s, labels, lse, gl, out=d)
        _, lse3 = ops.ce_kd_fwd(s, t, labels, 2.0, 1.0)
        ops.ce_kd_bwd(s, t, labels, lse3, 2.0, 1.0, gl, out=d)
        _, lse1 = ops.ce_mse_fwd(s, store, mi, labels, 0.5, 1.0)
        ops.ce_mse_bwd(s, store, mi, labels, lse1, 0.5, 1.0, gl, out=d)

    for i in range(SETS):
        once(i)
    torch.cuda.synchronize()
    with KernelProfile() as prof:
        for i in range(REPS):
            once(i)
    out = {}
    for tag, work, ms in prof.records():
        if tag in TAGS:
            out.setdefault(tag, {"us": [], "bytes": work})["us"].append(ms * 1e3)
    return out, B * T


def step_times(method_name, cfg, B, P, T, steps=12, warmup=4):
    from mafed_amd import DER, ER
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    n = 8 * B
    mem = samples(cfg, n, P, T, torch.Generator().manual_seed(1235))
    opts = types.SimpleNamespace(tasks=["t0", "t1"], batch_size=B, seed=1236, pin_mem=False, accumulate_grad_batches=1)
    if method_name == "naive":
        method = CLMethod["naive"]()
    else:
        method = (DER if method_name == "der" else ER)(opts, memory_size=n, model_type="vlpythia")
        method.update(mem, model=student)
        gen = torch.Generator(device=dev).manual_seed(1237)   # the student has moved away from the model that recorded the store
        with torch.no_grad():
            student.flat_params.add_(torch.randn(student.flat_params.shape, generator=gen, device=dev) * 1e-3)
        student._shadow_dirty = True
    tr = Trainer(student, method, step_conf("warmup_perc"), task_id=0 if method_name == "naive" else 1, n_batches_per_epoch=1000, pipeline_optimizer=True)
    ts, _, rec = run_steps(tr, to_dev({k: v[:B] for k, v in mem.items()}, sparse_head=True), steps, warmup)
    parts = f"  (last step: CE {float(method.last_ce):.4f}, MSE {float(method.last_mse):.3e})" if method_name == "der" else ""
    return ts, rec["branch"], float(rec["loss"]), parts


def recording_time(cfg, B, P, T, n=1000):
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    data = to_dev(samples(cfg, n, P, T, torch.Generator().manual_seed(1238)))

    def record():
        parts = [student.answer_logits(data["patch_embeddings"][lo:lo + B], data["input_ids"][lo:lo + B], data["attention_mask"][lo:lo + B],
                                       data["labels"][lo:lo + B], A) for lo in range(0, n, B)]
        return torch.cat(parts, dim=0)

    record()
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z = record()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, z.numel() * z.element_size()


def naive_only():
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    ts, branch, loss, _ = step_times("naive", cfg, B, P, T)
    print(f"{'naive':>12s} ({branch:>6s} branch): {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) ms   loss {loss:.4f}", flush=True)


def main():
    assert torch.cuda.is_available(), "der_bench needs a GPU"
    if "--naive-only" in sys.argv[1:]:
        return naive_only()
    print(header(__file__, sys.argv[1:]))
    print(f"# {torch.cuda.get_device_name(0)}; bf16 logits [rows, {V}], store [{N_MEM}, {A}, {V}] bf16; kernel time = the dispatch's own execution time, us, "
          f"median (min .. max) of {REPS}")
    print(f"{'rows':>5s} {'kernel':>11s} {'median us':>10s} {'min':>8s} {'max':>8s} {'MB':>8s} {'TB/s':>6s} {'vs ce_kd kernel':>16s}")
    store = torch.empty(N_MEM, A, V, dtype=torch.bfloat16, device=dev).normal_()
    for rows in (1024, 256):
        tm, real = kernel_times(rows, store)
        for tag, base in (("ce_fwd", None), ("ce_kd_fwd", None), ("ce_mse_fwd", "ce_kd_fwd"), ("ce_bwd", None), ("ce_kd_bwd", None), ("ce_mse_bwd", "ce_kd_bwd")):
            us = tm[tag]["us"]
            med = statistics.median(us)
            rel = f"{med / statistics.median(tm[base]['us']):16.2f}" if base else ""
            print(f"{real:5d} {tag:>11s} {med:10.1f} {min(us):8.1f} {max(us):8.1f} {tm[tag]['bytes'] / 1e6:8.1f} {tm[tag]['bytes'] / med / 1e6:6.2f} {rel}", flush=True)
    del store
    torch.cuda.empty_cache()
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    print(f"# VLPythia-410M bf16 step, B = {B}, {P} + {T} tokens, row-sparse head, pipelined optimiser; wall ms per Trainer.step, median (min .. max) of 12 after 4")
    for name in ("naive", "replay", "der"):
        ts, branch, loss, parts = step_times(name, cfg, B, P, T)
        print(f"{name:>12s} ({branch:>6s} branch): {statistics.median(ts):7.2f} ({min(ts):.2f} .. {max(ts):.2f}) ms   loss {loss:.4f}{parts}", flush=True)
        torch.cuda.empty_cache()
    ts, nbytes = recording_time(cfg, B, P, T)
    print(f"# one recording pass over 1000 samples in batches of {B} (model.answer_logits, A = {A}; a store of {nbytes / 1e6:.0f} MB): "
          f"{statistics.median(ts):.1f} ({min(ts):.1f} .. {max(ts):.1f}) ms, 3 passes after 1")
    torch.cuda.empty_cache()
    if "--parent-lib" in sys.argv[1:]:
        return parent_lib_ab(__file__, sys.argv[sys.argv.index("--parent-lib") + 1],
                             emit=lambda who, rnd, out: print(f"## {who}, round {rnd}\n{out.rstrip()}", flush=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
