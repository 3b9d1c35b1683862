"""The 410M MAFED replay step at text lengths that do and do not tile: ms per step and launches of the register-staged fallback GEMM per
step, with ``text_bucket`` 0 (the unpadded route) and "auto" (right padding to a tile multiple).

    python tools/ragged_bench.py [--out profiles/ragged_step.txt] [--steps 20] [--reps 3] [--rev <commit>]

B = 16 and B = 32, each for T in {23, 24, 29, 32}; P = 256.  One student / teacher / Trainer per batch size, the memory swapped per T.
Every figure is the median of ``--reps`` repetitions of ``--steps`` steps between two HIP events, with min .. max as the run-to-run spread.
Yardsticks: the ``text_bucket=0`` row of the same T (what the step did before), and the aligned row (T = 24 at B = 16, T = 32 at
B = 32), whose kernels the padded T = 23 / T = 29 step launches too.  Needs a GPU."""
import argparse
import os
import statistics
import subprocess
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_step.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--text-lengths", type=int, nargs="+", default=[23, 24, 29, 32])
    ap.add_argument("--model", default="410m")
    ap.add_argument("--rev", default=None, help="commit to name in the header (default: git rev-parse HEAD)")
    args = ap.parse_args()

    from mafed_amd import FeatureDistillation, Trainer, VLPythiaConfig, VLPythiaForCausalLM, ops
    from mafed_amd.methods import HBMReplayBuffer
    dev = torch.device("cuda:0")
    P = 256
    cfg = VLPythiaConfig.preset(args.model, num_vision_tokens=P)
    rev = args.rev
    if rev is None:
        try:
            rev = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            rev = "unknown"
    # (the command as it selects the measurement: where the table goes and the commit named below are not part of it)
    shown, skip = [], False
    for a in sys.argv[1:]:
        if skip or a in ("--out", "--rev"):
            skip = not skip
            continue
        if not a.startswith(("--out=", "--rev=")):
            shown.append(a)
    lines = ["# " + " ".join(["python", "tools/ragged_bench.py"] + shown),
             f"# git rev-parse HEAD: {rev}",
             f"# {torch.cuda.get_device_name(0)}; model {args.model}, P = {P}, bf16; {args.reps} x {args.steps} steps per row after {args.warmup} warm-up steps",
             "# ms/step: median of the repetitions (min .. max); fallback/step: launches of the register-staged GEMM per step",
             f"{'B':>3} {'T':>3} {'bucket':>6} {'T_run':>5} {'rows':>6} {'ms/step':>8} {'min':>8} {'max':>8} {'fallback/step':>13}"]
    print("\n".join(lines), flush=True)
    conf = types.SimpleNamespace(accumulate_grad_batches=1, replay_interval=1, grad_norm=2.0, learning_rate=5e-5, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_perc=0.1)
    for B in args.batch_sizes:
        student = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=dev, seed=1234)
        opts = types.SimpleNamespace(tasks=["t0", "t1"], batch_size=B, seed=1236, pin_mem=False, accumulate_grad_batches=1)
        fd = FeatureDistillation(memory_size=4000, opts=opts, model_type="vlpythia", num_hidden_layers=cfg.num_hidden_layers - 1,
                                 distillation_modality_weighing_strategy="balanced", distillation_layer_weighing_strategy="discounted",
                                 gamma=0.5, distillation_layer=None, distillation_coeff=1.0, replay_coeff=1.0)
        fd._update_model(student)
        g = torch.Generator(device=dev).manual_seed(1237)
        fd.past_model.flat_params.add_(torch.randn(fd.past_model.flat_params.shape, generator=g, device=dev) * 1e-3)
        fd.past_model._shadow_dirty = True
        fd.task_id, fd.num_vision_tokens = 1, P
        tr = Trainer(student, fd, conf, task_id=1, n_batches_per_epoch=1000, pipeline_optimizer=True)
        n_mem = 8 * B
        gcpu = torch.Generator().manual_seed(1235)
        feats = torch.randn(n_mem, P, cfg.vision_hidden_size, generator=gcpu).to(torch.bfloat16)
        for T in args.text_lengths:
            ids = torch.randint(1, cfg.vocab_size, (n_mem, T), generator=gcpu)
            labels = torch.full((n_mem, T), -100, dtype=torch.int64)
            labels[:, -4:] = ids[:, -4:]
            mem = HBMReplayBuffer(B, dev, seed=1236)
            mem.add({"input_ids": ids, "attention_mask": torch.ones(n_mem, T, dtype=torch.int64), "labels": labels, "patch_embeddings": feats})
            fd.mem_dataloader = mem
            task_batch = mem.sample()   # dropped by a replay step, as in the reference
            for bucket in (0, "auto"):
                student.text_bucket = fd.past_model.text_bucket = bucket
                T_run = student.padded_text_len(B, T)
                step = 0
                for _ in range(args.warmup):
                    tr.step(task_batch, step)
                    step += 1
                tr.join()
                torch.cuda.synchronize()
                ms, fb = [], []
                for _ in range(args.reps):
                    n0 = ops.gemm_fallback_launches()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        tr.step(task_batch, step)
                        step += 1
                    tr.join()
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1) / args.steps)
                    fb.append((ops.gemm_fallback_launches() - n0) / args.steps)
                row = (f"{B:>3} {T:>3} {str(bucket):>6} {T_run:>5} {B * (P + T_run):>6} {statistics.median(ms):>8.2f} {min(ms):>8.2f} {max(ms):>8.2f} "
                       f"{statistics.median(fb):>13.1f}")
                lines.append(row)
                print(row, flush=True)
        del tr, fd, student
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
