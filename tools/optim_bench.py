"""Per-pass time of the three optimiser rules (FlatAdamW / FlatAdam / FlatAdamax) on the flat buffers of a real VLPythia model (run on
the GPU box; profiles/optim_bench.txt).

Each rule owns its state buffers and runs over the same parameter / gradient / bf16 shadow buffers; one pass = the two weight-decay
segments (two launches), with and without the gradient zeroing.  Timed with device events around `--reps` back-to-back passes, after a
warm-up of every rule and form; the rules are alternated inside every round (order rotated per round) and the median over `--rounds`
is reported.  Bytes are algorithmic: p, m, v read + written, g read, the bf16 shadow written (30 B / parameter), + g written as zeros
(34 B / parameter); the rate is over the event time of the passes (kernels + launch boundaries), against the HBM figures of
MI355X_MICROARCH.md (8.0 TB/s peak, 6.29 TB/s measured float4 copy)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mafed_amd import FlatAdam, FlatAdamax, FlatAdamW, VLPythiaConfig, VLPythiaForCausalLM  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="410m")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench needs the GPU"
    cfg = VLPythiaConfig.preset(args.model, num_vision_tokens=256)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device="cuda", seed=1234)
    assert model.flat_shadow is not None
    n = model.flat_params.numel()
    gen = torch.Generator(device="cuda").manual_seed(0)
    grads = torch.randn(n, device="cuda", generator=gen) * 1e-3
    kw = dict(lr=5e-5, betas=(0.9, 0.98), weight_decay=0.01)
    opts = {"adamw": FlatAdamW(model, **kw), "adam": FlatAdam(model, **kw), "adamax": FlatAdamax(model, **kw)}
    for o in opts.values():
        o.advance()   # {lr, 1-b1^t, sqrt(1-b2^t)} of step 1 on the device; the passes below reuse them

    def pass_(rule, zero):
        opts[rule].apply(grad_mul=1.0, zero_grads=zero)

    for zero in (False, True):
        model.flat_grads.copy_(grads)
        for rule in opts:
            for _ in range(3):
                pass_(rule, zero)
    torch.cuda.synchronize()
    times = {(r, z): [] for r in opts for z in (False, True)}
    rules = list(opts)
    for rnd in range(args.rounds):
        order = rules[rnd % 3:] + rules[:rnd % 3]
        for zero in (False, True):
            model.flat_grads.copy_(grads)   # (the zeroing form leaves zeros behind; outside the timed window)
            for rule in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    pass_(rule, zero)
                e1.record()
                torch.cuda.synchronize()
                times[(rule, zero)].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    dev = torch.cuda.get_device_properties(0).name
    print(f"# tools/optim_bench.py --model {args.model} --reps {args.reps} --rounds {args.rounds}   ({dev}; {n / 1e6:.1f} M parameters, "
          f"bf16 shadow on)")
    print(f"# per pass = both weight-decay segments; median of {args.rounds} rounds of {args.reps} passes (min .. max)")
    print(f"{'rule':8s} {'form':9s} {'us/pass':>9s} {'range':>19s} {'B/param':>8s} {'GB':>6s} {'TB/s':>6s} {'% 8.0':>6s} {'% 6.29':>7s} {'vs adamw':>9s}")
    for zero in (False, True):
        bpp = 34 if zero else 30
        base = statistics.median(times[("adamw", zero)])
        for rule in rules:
            t = times[(rule, zero)]
            med = statistics.median(t)
            rate = bpp * n / (med * 1e-6)
            print(f"{rule:8s} {'zero_grad' if zero else 'keep_grad':9s} {med:9.1f} {min(t):9.1f} .. {max(t):7.1f} {bpp:8d} {bpp * n / 1e9:6.2f} "
                  f"{rate / 1e12:6.2f} {100 * rate / HBM_PEAK:5.1f}% {100 * rate / HBM_COPY:6.1f}% {100 * (med / base - 1):+8.1f}%")


if __name__ == "__main__":
    main()
