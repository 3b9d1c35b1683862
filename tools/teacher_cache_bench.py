"""What the teacher cache costs and saves per optimiser step (run on the GPU box; profiles/teacher_cache_compact.txt).

The bench's MAFED step (bf16 compute, synthetic inputs of bench.py, B = 32, 256 + 32 tokens) with
  none    no cache: the frozen teacher's forward runs in every replay step
  fp32    the fp32 cache
  bf16    the bf16 cache (``teacher_cache_dtype="bf16"``: half the memory, the distillation target rounded to bf16)
alternated inside ONE process: every case of a round runs `--reps` timed steps (host clock around the steps + a device
synchronise, as bench.py times its legs) after two untimed ones, the order of the cases is rotated per round, and the median over
`--rounds` is reported with its range -- the range of a case over the rounds is its run-to-run spread on that box.

`--repo DIR` imports mafed_amd from another checkout (built there), e.g. the parent commit: a checkout whose
``build_teacher_cache`` has no ``dtype`` argument is the one that gathers a dense fp32 copy of the batch's rows per step; its cases
are ``none`` and ``fp32``.  Two processes on the same box share the ``none`` case, which ties their clocks together.

`--fit` (with a larger `--model`): instead of `--memory-size`, the replay memory is as large as the bf16 cache that fits beside the
model, its Adam state and a step's activations (free HBM after a step, minus `--margin-gb`), capped at `--memory-size`; reports the
number of samples next to the fp32 figure from the same arithmetic.
"""
import argparse
import inspect
import os
import statistics
import subprocess
import sys
import time
import types

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default=None, help="names the checkout in the table (default: git rev-parse HEAD of --repo, if it is a git checkout)")
ap.add_argument("--model", default="410m")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--memory-size", type=int, default=4000)
ap.add_argument("--cases", default=None, help="comma-separated subset of none,fp32,bf16")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--fit", action="store_true")
ap.add_argument("--margin-gb", type=float, default=16.0)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))

import torch  # noqa: E402

from mafed_amd import FeatureDistillation, Trainer, VLPythiaConfig, VLPythiaForCausalLM  # noqa: E402
from mafed_amd.methods import HBMReplayBuffer  # noqa: E402


def rev():
    if args.label:
        return args.label
    try:
        return subprocess.run(["git", "-C", args.repo, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    assert torch.cuda.is_available(), "teacher_cache_bench needs the GPU"
    dev = torch.device("cuda", 0)
    B, P, T = args.batch, 256, 32
    cfg = VLPythiaConfig.preset(args.model, num_vision_tokens=P)
    student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
    opts = types.SimpleNamespace(tasks=["t0", "t1"], batch_size=B, seed=1236, pin_mem=False, accumulate_grad_batches=1)
    fd = FeatureDistillation(memory_size=4000, opts=opts, model_type="vlpythia", num_hidden_layers=cfg.num_hidden_layers - 1,
                             distillation_modality_weighing_strategy="balanced", distillation_layer_weighing_strategy="discounted",
                             gamma=0.5, distillation_layer=None, distillation_coeff=1.0, replay_coeff=1.0)
    fd._update_model(student)
    g = torch.Generator(device=dev).manual_seed(1237)
    fd.past_model.flat_params.add_(torch.randn(fd.past_model.flat_params.shape, generator=g, device=dev) * 1e-3)
    fd.past_model._shadow_dirty = True
    fd.task_id = 1
    fd.num_vision_tokens = P
    has_dtype = "dtype" in inspect.signature(fd.build_teacher_cache).parameters
    cases = args.cases.split(",") if args.cases else (["none", "fp32", "bf16"] if has_dtype else ["none", "fp32"])
    assert has_dtype or "bf16" not in cases, "this checkout has no bf16 teacher cache"
    conf = types.SimpleNamespace(accumulate_grad_batches=1, replay_interval=1, grad_norm=2.0, learning_rate=5e-5, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_perc=0.1)

    def memory(n):
        gcpu = torch.Generator().manual_seed(1235)
        ids = torch.randint(1, cfg.vocab_size, (n, T), generator=gcpu)
        labels = torch.full((n, T), -100, dtype=torch.int64)
        labels[:, -4:] = ids[:, -4:]
        gmem = torch.Generator(device=dev).manual_seed(1234)
        feats = torch.empty(n, P, cfg.vision_hidden_size, dtype=torch.bfloat16, device=dev)
        for lo in range(0, n, 512):
            hi = min(n, lo + 512)
            feats[lo:hi] = torch.randn(hi - lo, P, cfg.vision_hidden_size, generator=gmem, device=dev).to(torch.bfloat16)
        mem = HBMReplayBuffer(B, dev, seed=1236)
        mem.add({"input_ids": ids, "attention_mask": torch.ones(n, T, dtype=torch.int64), "labels": labels, "patch_embeddings": feats})
        return mem

    layers = len(fd.loss_weights.get_distillation_layers())
    per_sample = {"fp32": layers * (P + T) * cfg.hidden_size * 4, "bf16": layers * (P + T) * cfg.hidden_size * 2}
    n_mem, fit = max(8 * B, args.memory_size), None
    mem = memory(8 * B if args.fit else n_mem)
    fd.mem_dataloader = mem
    tr = Trainer(student, fd, conf, task_id=1, n_batches_per_epoch=1000, pipeline_optimizer=True, incremental_norm=True)
    task_batch = mem.sample()
    step_no = [0]

    def steps(n):
        for _ in range(n):
            rec = tr.step(task_batch, step_no[0])
            step_no[0] += 1
        torch.cuda.synchronize()
        return rec

    steps(3)    # the model's, the optimiser's and a step's own allocations are made
    if args.fit:
        tr.join()
        torch.cuda.empty_cache()
        free, total = torch.cuda.mem_get_info(dev)
        feat_bytes = P * cfg.vision_hidden_size * 2 + 3 * T * 8
        room = free - int(args.margin_gb * 2 ** 30)
        fit = {k: max(0, room // (v + feat_bytes)) for k, v in per_sample.items()}
        n_mem = max(8 * B, min(args.memory_size, int(fit["bf16"])))
        cases = [c for c in cases if c != "fp32" or n_mem <= fit["fp32"]]
        mem = memory(n_mem)
        fd.mem_dataloader = mem
        task_batch = mem.sample()

    caches, info = {"none": None}, {}
    for c in cases:
        if c == "none":
            continue
        info[c] = fd.build_teacher_cache(mem, dtype=c) if has_dtype else fd.build_teacher_cache(mem)
        caches[c] = fd._tcache
    ms = {c: [] for c in cases}
    loss = {}

    def select(c):
        tr.join()
        fd._tcache = caches[c]
        mem.attach_index = caches[c] is not None
        mem._next = None       # a batch gathered ahead carries the previous case's index (or none)

    for c in cases:
        select(c)
        steps(3)
    for rnd in range(args.rounds):
        k = rnd % len(cases)
        for c in cases[k:] + cases[:k]:
            select(c)
            steps(2)
            t0 = time.perf_counter()
            rec = steps(args.reps)
            ms[c].append((time.perf_counter() - t0) * 1e3 / args.reps)
            loss[c] = float(rec["loss"])
            assert loss[c] == loss[c], f"NaN loss in case {c}"
    name = torch.cuda.get_device_properties(0).name
    print(f"# python {' '.join(['tools/teacher_cache_bench.py'] + sys.argv[1:])}   (checkout {rev()}; {time.strftime('%Y-%m-%d')}; {name})")
    print(f"# {args.model}, B = {B}, {P} + {T} tokens, bf16 compute, {layers} distilled layers, replay memory {n_mem} samples; "
          f"median of {args.rounds} rounds of {args.reps} steps (min .. max); the cases continue ONE training run, so their last losses are not comparable")
    if fit is not None:
        print(f"# free HBM after a step {free / 1e9:.1f} of {total / 1e9:.1f} GB, margin {args.margin_gb:.0f} GB: a bf16 cache fits {int(fit['bf16'])} samples "
              f"({per_sample['bf16'] / 1e6:.1f} MB each), an fp32 cache {int(fit['fp32'])} ({per_sample['fp32'] / 1e6:.1f} MB each) by the same arithmetic")
    how = {"none": "teacher forward", "fp32": "read in place" if has_dtype else "gathered copy", "bf16": "read in place"}
    print(f"{'case':6s} {'teacher states':16s} {'ms/step':>8s} {'range':>17s} {'samples/s':>10s} {'cache GB':>9s} {'fill s':>7s} {'vs none':>8s} {'last loss':>9s}")
    base = statistics.median(ms["none"]) if "none" in ms else None
    for c in cases:
        med = statistics.median(ms[c])
        gb = f"{info[c]['GB']:9.1f}" if c in info else f"{'-':>9s}"
        fill = f"{info[c]['seconds']:7.1f}" if c in info else f"{'-':>7s}"
        rel = f"{100 * (med / base - 1):+7.1f}%" if base else f"{'-':>8s}"
        print(f"{c:6s} {how[c]:16s} {med:8.2f} {min(ms[c]):7.2f} .. {max(ms[c]):6.2f} {B / med * 1e3:10.1f} {gb} {fill} {rel} {loss[c]:9.5f}")


if __name__ == "__main__":
    main()
