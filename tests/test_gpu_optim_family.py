"""GPU: torch.optim.Adam / Adamax on the flat buffers (mafed_adam_step / mafed_adamax_step, FlatAdam / FlatAdamax, Trainer optim =
"adam" / "adamax") against torch itself -- fp64 on the CPU for the kernels, a CPU restatement of the MAFED training sequence from the
oracle's pieces for the Trainer (the optimiser built exactly as configure_optimizers builds it: two groups, lr and betas only)."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import vlpythia_ref as R
from tests.helpers import TINY, load_golden, tiny_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
RULES = {"adam": torch.optim.Adam, "adamax": torch.optim.Adamax}
SECOND = {"adam": "exp_avg_sq", "adamax": "exp_inf"}


def close(a, b, tol, what=""):
    a = np.asarray(a.detach().cpu().double() if isinstance(a, torch.Tensor) else a, np.float64)
    b = np.asarray(b.detach().cpu().double() if isinstance(b, torch.Tensor) else b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    scale = max(1.0, np.abs(b).max() if b.size else 1.0)
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e}*{scale:.3g}"


def build_model(cfg, sd, dtype=torch.float32):
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    mc = VLPythiaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        vision_hidden_size=cfg.vision_hidden_size, num_vision_tokens=cfg.num_vision_tokens)
    m = VLPythiaForCausalLM(mc, compute_dtype=dtype, device=DEV)
    m.load_state_dict(sd, strict=True)
    return m


def to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


# ---- 0. the piecewise clip norm at the sizes of the flat-buffer passes ----------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4 * 1024 + 1, 3 * 2 ** 21 + 5])
def test_gradnorm_partial_and_finish_vs_one_pass_and_fp64(n):
    """The sizes of tests/test_gpu_si.py: tail only (twice), one vector, less than one block, several blocks and a tail, and a grid at
    its cap (1024 blocks here) that takes more than one two-vector trip; without 0, since gradnorm_partial refuses an empty tensor's
    null pointer.  Exactly gradnorm_blocks(n) partials are written, run to run the same bits, and their fold equals the one-pass norm
    and float64 to 1e-6."""
    from mafed_amd import ops
    g = torch.randn(n, generator=torch.Generator().manual_seed(3000 + n % 997)).to(DEV)
    nb = ops.gradnorm_blocks(n)
    partials, again = torch.full((nb + 3,), -7.0, device=DEV), torch.full((nb + 3,), -7.0, device=DEV)
    ops.gradnorm_partial(g, partials)
    ops.gradnorm_partial(g, again)
    assert 1 <= nb <= 1024 and bool((partials[nb:] == -7.0).all()) and torch.equal(partials.view(torch.int32), again.view(torch.int32))
    folded = ops.gradnorm_finish(partials[:nb], 2.0, torch.empty(2, device=DEV))
    ref64 = float(g.double().square().sum().sqrt())
    print(f"[gradnorm] n {n}: {nb} partials, norm {float(folded[0]):.8g} (fp64 {ref64:.8g})")
    one_pass = ops.gradnorm_clip(g, 2.0)
    for i, what in enumerate(("norm", "clip scale")):
        a, b = float(folded[i]), float(one_pass[i])
        assert abs(a - b) <= 1e-6 * abs(b), f"{what}: folded {a} vs one pass {b}"
    assert abs(float(folded[0]) - ref64) <= 1e-6 * ref64


# ---- 1. the kernels against torch in fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", list(RULES))
def test_kernel_vs_torch_fp64(rule):
    """A decayed (1003) and a non-decayed (517) segment -- neither a multiple of 4 -- of one flat buffer, with a 5-element gap between
    them that no launch may touch; 5 steps of random gradients, grad_mul 0.25, the clip from the norm kernel (steps 2 and 4 clipped),
    the scalars from the device advance under a warm-up schedule.  p and both state buffers within 2e-6 of torch in fp64, the bf16
    shadow = p.to(bfloat16) bit for bit."""
    from mafed_amd import ops
    nA, offB, nB = 1003, 1008, 517
    N = offB + nB
    lr, b1, b2, eps, wd, max_norm, warm, total = 1e-2, 0.9, 0.999, 1e-8, 0.05, 8.0, 2, 10
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(N, generator=gen)
    p = p0.to(DEV)
    m, s = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    sh = torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    state = torch.zeros(1, dtype=torch.int64, device=DEV)
    hyper = torch.tensor([lr, 1.0, 1.0], device=DEV)
    clip = torch.zeros(2, device=DEV)
    segs = [(0, nA, wd), (offB, N, 0.0)]

    ref = [p0[lo:hi].double().clone() for lo, hi, _ in segs]
    opt = RULES[rule]([{"params": [ref[0]], "weight_decay": wd}, {"params": [ref[1]], "weight_decay": 0.0}], lr=lr, betas=(b1, b2), eps=eps)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda st: R.lr_lambda(st, warm, total))
    clipped = 0
    for step in range(5):
        g = torch.randn(N, generator=gen) * (0.6 if step % 2 else 0.05)
        g[nA:offB] = 0.0
        gd = g.to(DEV)
        ops.gradnorm_clip(gd, max_norm, clip)
        ops.optim_advance_(state, lr, warm, total, b1, b2, hyper, clip=clip)
        for lo, hi, w in segs:
            ops.adam_family_step_(rule, p[lo:hi], gd[lo:hi], m[lo:hi], s[lo:hi], hyper, b1, b2, eps, w, 0, clip, 0.25, sh[lo:hi])
        norm = float(torch.linalg.vector_norm(g.double()))
        scale = min(1.0, max_norm / (norm + 1e-6))
        clipped += scale < 1.0
        for t, (lo, hi, _) in zip(ref, segs):
            t.grad = g[lo:hi].double() * 0.25 * scale
        opt.step()
        sch.step()
    assert clipped == 2
    torch.cuda.synchronize()
    assert int(state) == 5
    for t, (lo, hi, _) in zip(ref, segs):
        st = opt.state[t]
        for what, got, want in (("p", p[lo:hi], t), ("exp_avg", m[lo:hi], st["exp_avg"]), (SECOND[rule], s[lo:hi], st[SECOND[rule]])):
            err = float((got.cpu().double() - want).abs().max())
            assert err <= 2e-6 * float(want.abs().max()), f"{rule} [{lo}, {hi}) {what}: {err:.3e}"
        assert torch.equal(sh[lo:hi], p[lo:hi].to(torch.bfloat16))
    assert torch.equal(p[nA:offB].cpu(), p0[nA:offB]) and float(m[nA:offB].abs().max()) == 0.0 and float(s[nA:offB].abs().max()) == 0.0
    assert float(sh[nA:offB].float().abs().max()) == 0.0


# ---- 2. zeroing forms, the host-step form, the skipped step --------------------------------------------------------------------
@pytest.mark.parametrize("rule", list(RULES))
def test_zeroing_forms_and_skip(rule):
    """zero_n = 0 / 500 / n: the same update, only g[0, zero_n) zeroed; step = t on the host gives the device form's result bit for bit;
    a NaN in g: clip scale -1, p / m / state bit-identical, the counter stands, g still zeroed where asked."""
    from mafed_amd import _lib, ops
    n, b1, b2, eps, wd = 1003, 0.9, 0.98, 1e-8, 0.01
    gen = torch.Generator(device=DEV).manual_seed(3)
    p0, g0 = torch.randn(n, device=DEV, generator=gen), torch.randn(n, device=DEV, generator=gen)
    m0, s0 = torch.randn(n, device=DEV, generator=gen) * 0.1, torch.rand(n, device=DEV, generator=gen) * 0.01 + 1e-3
    state = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    hyper = torch.zeros(3, device=DEV)
    clip = torch.zeros(2, device=DEV)
    ops.gradnorm_clip(g0, 20.0, clip)
    ops.optim_advance_(state, 1e-2, 0, 0, b1, b2, hyper, clip=clip)
    assert int(state) == 3

    def run(zero_n, step=0, g=g0, clip_t=clip):
        p, gg, m, s = p0.clone(), g.clone(), m0.clone(), s0.clone()
        sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        ops.adam_family_step_(rule, p, gg, m, s, hyper, b1, b2, eps, wd, step, clip_t, 1.0, sh, zero_n=zero_n)
        return p, gg, m, s, sh

    full = run(0)
    assert torch.equal(full[1], g0) and not torch.equal(full[0], p0)
    for zn in (500, n):
        out = run(zn)
        for i in (0, 2, 3, 4):
            assert torch.equal(out[i], full[i]), (zn, i)
        assert float(out[1][:zn].abs().max()) == 0.0 and torch.equal(out[1][zn:], g0[zn:])
    host = run(0, step=3)
    for i in range(5):
        assert torch.equal(host[i], full[i]), i
    with pytest.raises(_lib.MafedHipError):
        run(501)   # a partial zero_n must keep the 16-byte stores aligned

    bad = g0.clone()
    bad[123] = float("nan")
    ops.gradnorm_clip(bad, 20.0, clip)
    ops.optim_advance_(state, 1e-2, 0, 0, b1, b2, hyper, clip=clip)
    torch.cuda.synchronize()
    assert float(clip[1]) < 0 and int(state) == 3
    for zn in (0, 500, n):
        p, gg, m, s, sh = run(zn, g=bad)
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(s, s0) and float(sh.float().abs().max()) == 0.0
        assert torch.equal(gg.view(torch.int32)[zn:], bad.view(torch.int32)[zn:]) and int(torch.count_nonzero(gg[:zn])) == 0


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("pipeline", [False, True])
def test_trainer_bf16_overwrite_and_nonfinite_skip(rule, pipeline):
    """The bf16 perf path -- overwrite-mode weight gradients, fused matrix squares in the incremental norm -- equals the classic
    "zero, then accumulate" steps under the new rules too; a NaN loss leaves parameters and state alone and does not advance the step."""
    from mafed_amd import Trainer
    from mafed_amd.methods import Naive
    cfg = tiny_cfg("t64")
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    batches = [to_dev(R.make_batch(cfg, 4, 6, seed=60 + i, pad=True, n_answer=3)) for i in range(4)]
    conf = types.SimpleNamespace(accumulate_grad_batches=2, replay_interval=1, grad_norm=2.0, learning_rate=1e-3, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim=rule, warmup_steps=0, total_steps=100)
    runs = []
    for overwrite in (True, False):
        student = build_model(cfg, sd, torch.bfloat16)
        student.dw_group_layers = 2
        tr = Trainer(student, Naive(), conf, task_id=0, pipeline_optimizer=pipeline, overwrite_weight_grads=overwrite)
        assert tr._overwrite_ok() == overwrite and type(tr.optimizer).__name__ == {"adam": "FlatAdam", "adamax": "FlatAdamax"}[rule]
        for i, b in enumerate(batches):
            tr.step(dict(b), i)
        tr.join()
        torch.cuda.synchronize()
        runs.append((student, tr))
    (a, tra), (b, _) = runs
    assert int(tra.optimizer.state_dev) == 2 and a._dw_stale
    d = float((a.flat_params - b.flat_params).abs().max())
    assert d <= 2e-5, f"overwrite vs zero-then-accumulate: parameters differ by {d}"
    # a NaN loss on the next window: nothing moves
    p1, m1 = a.flat_params.clone(), tra.optimizer.exp_avg.clone()
    s1 = getattr(tra.optimizer, SECOND[rule]).clone()
    hook = a.register_forward_hook(lambda mod, args, out: setattr(out, "loss", out.loss * float("nan")) or out)
    tra.step(dict(batches[0]), 4)
    rec = tra.step(dict(batches[1]), 5)
    hook.remove()
    tra.join()
    torch.cuda.synchronize()
    assert rec["stepped"] and not torch.isfinite(rec["grad_norm"]).item()
    assert torch.equal(a.flat_params, p1) and torch.equal(tra.optimizer.exp_avg, m1) and torch.equal(getattr(tra.optimizer, SECOND[rule]), s1)
    assert int(tra.optimizer.state_dev) == 2, "the device step counter advanced on a skipped step"
    assert float(a.flat_grads[a.decay_split():].abs().max()) == 0.0


# ---- 3. the Trainer's MAFED sequence against a CPU restatement -----------------------------------------------------------------
def _fd(cfg, teacher, t):
    from mafed_amd import FeatureDistillation
    opts = types.SimpleNamespace(tasks=["a", "b", "c"], batch_size=t["B"], seed=42, pin_mem=False, accumulate_grad_batches=4)
    fd = FeatureDistillation(memory_size=100, opts=opts, model_type="vlpythia", num_hidden_layers=cfg.num_hidden_layers - 1,
                             distillation_modality_weighing_strategy="balanced", distillation_layer_weighing_strategy="discounted",
                             gamma=0.5, distillation_layer=None, distillation_coeff=1.0, replay_coeff=1.0)
    fd._update_model(teacher)
    fd.task_id = 1
    fd.num_vision_tokens = cfg.num_vision_tokens
    return fd


def _scenario():
    g = load_golden("trainer_t64.npz")
    seed = int(g["meta/seed"])
    cfg, t = tiny_cfg("t64"), TINY["t64"]
    sd = R.init_weights(cfg, seed=seed, bias_std=0.02, ln_jitter=0.05)
    tsd = R.perturb(sd, seed=seed + 100, std=5e-3)
    batches = [(R.make_batch(cfg, t["B"], t["T"], seed=seed + 10 + bi, pad=True, n_answer=3),
                R.make_batch(cfg, t["B"], t["T"], seed=seed + 50 + bi, pad=True, n_answer=3)) for bi in range(8)]
    # (no warm-up: with the golden's 2 steps the first update has lr 0, and the losses after it would not depend on the rule)
    meta = dict(lr=float(g["meta/lr"]), warmup=0, total=int(g["meta/total_steps"]))
    return cfg, t, sd, tsd, batches, meta


@functools.lru_cache(maxsize=None)
def _cpu_sequence(rule):
    """The reference's training sequence on the CPU in fp32 with torch's own optimiser: replay / distillation every 4th micro-batch,
    accumulate 4, clip 2.0, then ``OptimCls(groups, lr=..., betas=...)`` + get_linear_schedule_with_warmup, as configure_optimizers."""
    cfg, t, sd, tsd, batches, meta = _scenario()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    names = list(params)
    assert all(R.param_group_of(k) >= 2 for k in names)   # the lr_mul "vqa_output" groups are empty for VLPythia
    groups = [{"params": [params[k] for k in names if R.param_group_of(k) == 2], "weight_decay": 0.01},
              {"params": [params[k] for k in names if R.param_group_of(k) == 3], "weight_decay": 0.0}]
    opt = RULES[rule](groups, lr=meta["lr"], betas=(0.9, 0.98))
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda st: R.lr_lambda(st, meta["warmup"], meta["total"]))
    spec = R.DistillSpec(modality="balanced", layer_strategy="discounted", gamma=0.5, distillation_layer=None,
                         distillation_coeff=1.0, replay_coeff=1.0)
    out = {"branch": [], "loss": [], "grad_norm": [], "lr": [], "checksum": []}
    for bi, (batch, mem) in enumerate(batches):
        if (bi + 1) % 4 == 0:
            loss, _, _ = R.mafed_replay_loss(params, tsd, mem, cfg, spec, task_id=1)
            out["branch"].append(1)
        else:
            loss = R.forward(params, batch, cfg).loss
            out["branch"].append(0)
        out["loss"].append(float(loss.detach()))
        (loss / 4).backward()
        if (bi + 1) % 4 == 0:
            grads = [params[k].grad for k in names]
            total, scale = R.clip_grad_norm(grads, 2.0)
            for gr in grads:
                gr.mul_(scale)
            out["grad_norm"].append(float(total))
            out["lr"].append(opt.param_groups[0]["lr"])
            opt.step()
            sch.step()
            opt.zero_grad(set_to_none=True)
            out["checksum"].append(float(sum(p.detach().double().sum() for p in params.values())))
    return {k: np.array(v, np.float64) for k, v in out.items()}


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("mode", ["eager", "pipeline", "reducer"])
def test_trainer_sequence_vs_cpu_restatement(rule, mode):
    """test_trainer_sequence_vs_reference_golden's scenario (t64, task 1, FeatureDistillation balanced / discounted, replay_interval 4,
    accumulate 4, 8 micro-batches) with optim = "adam" / "adamax": branch, loss, grad norm, lr and parameter checksum after each
    optimiser step, at that test's tolerances.  "reducer": the GradReducer path (one-rank emulated exchange, one-pass clip norm)."""
    from mafed_amd import Trainer
    from mafed_amd.dist import EmulatedReducer
    ref = _cpu_sequence(rule)
    cfg, t, sd, tsd, batches, meta = _scenario()
    model, teacher = build_model(cfg, sd), build_model(cfg, tsd)
    fd = _fd(cfg, teacher, t)
    conf = types.SimpleNamespace(accumulate_grad_batches=4, replay_interval=4, grad_norm=2.0, learning_rate=meta["lr"], betas=(0.9, 0.98),
                                 weight_decay=0.01, optim=rule, warmup_steps=meta["warmup"], total_steps=meta["total"])
    pipeline = mode == "pipeline"
    reducer = EmulatedReducer(model, allreduce_ms=0.01, channels=1, world=1, buffer_mb=1) if mode == "reducer" else None
    tr = Trainer(model, fd, conf, task_id=1, pipeline_optimizer=pipeline, reducer=reducer)
    assert tr.optimizer.eps == 1e-8 and tr.optimizer.betas == (0.9, 0.98)
    branches, losses, gns, lrs, sums = [], [], [], [], []
    for bi, (batch, mem) in enumerate(batches):
        fd.mem_dataloader = [to_dev(mem)]
        rec = tr.step(to_dev(batch), bi)
        branches.append(int(rec["branch"] == "replay"))
        losses.append(float(rec["loss"]))
        if rec["stepped"]:
            gns.append(float(rec["grad_norm"]))
            lrs.append(rec["lr"])
            if pipeline and bi == 3:
                assert model._param_events is not None
            else:
                tr.join()
                sums.append(float(sum(p.detach().double().sum() for p in model.parameters())))
                assert float(model.flat_grads.abs().max()) == 0.0
    tr.join()
    assert branches == list(ref["branch"].astype(int))
    close(np.array(losses), ref["loss"], 1e-3, "loss sequence")
    close(np.array(gns), ref["grad_norm"], 1e-3, "grad-norm sequence")
    close(np.array(lrs), ref["lr"], 1e-9, "lr sequence")
    close(np.array(sums), ref["checksum"][-len(sums):], 1e-5, "parameter checksum after each optimiser step")


# ---- 4. optimiser state ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", list(RULES))
def test_state_dict_resume_is_bit_identical(rule):
    """state_dict after 2 optimiser steps, loaded into a fresh Trainer over a model holding the same parameters: the next 2 steps give
    bit-identical parameters to the uninterrupted run."""
    from mafed_amd import Trainer
    cfg, t, sd, tsd, batches, meta = _scenario()
    conf = types.SimpleNamespace(accumulate_grad_batches=1, replay_interval=4, grad_norm=2.0, learning_rate=meta["lr"], betas=(0.9, 0.98),
                                 weight_decay=0.01, optim=rule, warmup_steps=1, total_steps=20)

    def trainer(params):
        model = build_model(cfg, params)
        fd = _fd(cfg, build_model(cfg, tsd), t)
        return model, fd, Trainer(model, fd, conf, task_id=1)

    def run(model, fd, tr, steps):
        for bi in steps:
            batch, mem = batches[bi]
            fd.mem_dataloader = [to_dev(mem)]
            tr.step(to_dev(batch), bi)
        tr.join()
        torch.cuda.synchronize()

    model, fd, tr = trainer(sd)
    run(model, fd, tr, [0, 1])
    saved_params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    saved_opt = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in tr.optimizer.state_dict().items()}
    assert saved_opt["optim"] == rule and saved_opt["step"] == 2 and SECOND[rule] in saved_opt
    run(model, fd, tr, [2, 3])
    model2, fd2, tr2 = trainer(saved_params)
    tr2.optimizer.load_state_dict(saved_opt)
    run(model2, fd2, tr2, [2, 3])
    assert int(tr2.optimizer.state_dev) == 4
    assert torch.equal(model2.flat_params, model.flat_params)
    assert torch.equal(getattr(tr2.optimizer, SECOND[rule]), getattr(tr.optimizer, SECOND[rule]))


def test_foreign_state_and_unknown_optimiser_are_refused():
    from mafed_amd import FlatAdam, FlatAdamax, FlatAdamW, Naive, Trainer
    cfg, t, sd, tsd, batches, meta = _scenario()
    model = build_model(cfg, sd)
    with pytest.raises(ValueError):
        FlatAdam(model).load_state_dict(FlatAdamW(model).state_dict())
    with pytest.raises(ValueError):
        FlatAdamax(model).load_state_dict(FlatAdam(model).state_dict())
    with pytest.raises(ValueError, match="invalid optimizer"):
        Trainer(model, Naive(), types.SimpleNamespace(optim="sgd"))
