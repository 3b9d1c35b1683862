"""Synaptic Intelligence (mafed_amd/methods/si.py, csrc/si.hip): the three flat-buffer passes against float64 numpy, and the plugin's life
inside Trainer.step -- task 0 against Naive, a task boundary against a float64 torch twin, the bf16 default Trainer with the pipelined
optimiser, a skipped step and the refusals."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import assert_rel_close, golden_setup, trainer_case
from tests.si_ref import SI_TRAINER, make_torch_si, si_accumulate_fp64, si_consolidate_fp64, si_stash_fp64, si_trainer_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3   # the project's fp32 gate
EPS22, EPS21 = 2.0 ** -22, 2.0 ** -21

# 0: empty; 1, 3: tail only; 4: one vector; 1023: less than one block; 4 * 1024 + 1: several blocks and a tail behind full vectors;
# 3 * 2^21 + 5: above 2 * 2048 * 256 * 4, so the grid-stride loop at the grid cap goes through its two-accumulator body and on
SIZES = [0, 1, 3, 4, 1023, 4 * 1024 + 1, 3 * 2 ** 21 + 5]
TWO_C, XI = 1.5, 1e-3

_INPUTS = {}


def _inputs(n):
    """{g, p, omega, anchor, w} fp32 on the device; built once per size and left unchanged.  g carries a -0.0."""
    if n not in _INPUTS:
        gen = torch.Generator().manual_seed(2000 + n % 997)
        g, p, w = (torch.randn(n, generator=gen) for _ in range(3))
        if n > 2:
            g[2] = -0.0
        anchor = p + 0.05 * torch.randn(n, generator=gen)
        omega = torch.randn(n, generator=gen).abs()
        _INPUTS[n] = {k: v.to(DEV) for k, v in dict(g=g, p=p, omega=omega, anchor=anchor, w=w).items()}
    return _INPUTS[n]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.double().cpu().numpy()


def _stash(x, penalty):
    from mafed_amd import ops
    n = x["g"].numel()
    g = x["g"].clone()
    sg, sp = torch.full_like(g, 3.0), torch.full_like(g, 3.0)
    nb = ops.si_blocks(n)
    sumsq, pen = torch.full((nb + 3,), -7.0, device=DEV), torch.full((nb + 3,), -7.0, device=DEV)
    ops.si_stash(g, x["p"], x["omega"] if penalty else None, x["anchor"] if penalty else None, TWO_C, sg, sp, sumsq, pen)
    return g, sg, sp, sumsq, pen, nb


@pytest.mark.parametrize("penalty", [False, True], ids=["task0", "penalty"])
@pytest.mark.parametrize("n", SIZES)
def test_si_stash_vs_fp64(n, penalty):
    from mafed_amd import ops
    x = _inputs(n)
    g, sg, sp, sumsq, pen, nb = _stash(x, penalty)
    again = _stash(x, penalty)
    torch.cuda.synchronize()
    for a, b in zip((g, sg, sp, sumsq, pen), again):   # run to run: the same bits
        assert torch.equal(_bits(a), _bits(b))
    assert 1 <= nb <= 2048 and bool((sumsq[nb:] == -7.0).all()) and bool((pen[nb:] == -7.0).all())
    # the stashes are bit copies (the -0.0 in g[2] stays -0.0)
    assert torch.equal(_bits(sg), _bits(x["g"])) and torch.equal(_bits(sp), _bits(x["p"]))
    want, term, pen64 = si_stash_fp64(_np(x["g"]), _np(x["p"]), _np(x["omega"]) if penalty else None, _np(x["anchor"]) if penalty else None, TWO_C)
    if penalty:
        err = np.abs(_np(g) - want)
        bound = EPS22 * (np.abs(_np(x["g"])) + np.abs(term))
        assert bool((err <= bound).all()), f"g': worst excess {float((err - bound).max()):.3e}"
        if n:
            assert not torch.equal(g, x["g"])
    else:
        assert torch.equal(_bits(g), _bits(x["g"]))   # only read
        assert bool((pen[:nb] == 0.0).all())
    # norm hand-over: the partials folded by gradnorm_finish against the one-pass norm of the g it left, and against float64
    folded = ops.gradnorm_finish(sumsq[:nb], 2.0, torch.empty(2, device=DEV))
    ref64 = float(np.sqrt((_np(g) ** 2).sum()))
    if n:
        one_pass = ops.gradnorm_clip(g, 2.0)
        for i, what in enumerate(("norm", "clip scale")):
            a, b = float(folded[i]), float(one_pass[i])
            assert abs(a - b) <= 1e-6 * abs(b), f"{what}: folded {a} vs one pass {b}"
        assert abs(float(folded[0]) - ref64) <= 1e-6 * ref64
    else:
        assert float(folded[0]) == 0.0 and float(folded[1]) == 1.0
    # last_penalty = c sum Omega (p - p*)^2: non-negative terms, about 40 fp32 additions per chain, then double
    c = TWO_C / 2
    got = float(ops.si_penalty_finish(pen[:nb], c))
    print(f"[si] n {n} {'penalty' if penalty else 'task0'}: norm {float(folded[0]):.8g} (fp64 {ref64:.8g}), penalty {got:.8g} (fp64 {c * pen64:.8g})")
    assert abs(got - c * pen64) <= 1e-5 * c * pen64
    if not penalty or n == 0:
        assert got == 0.0


def _moved(x):
    """(stash_g, stash_p, p): every third element did not move and has inf / NaN in its stashed gradient."""
    n = x["g"].numel()
    idx = torch.arange(n, device=DEV)
    still = idx % 3 == 0
    gen = torch.Generator(device=DEV).manual_seed(77 + n % 997)
    p = torch.where(still, x["p"], x["p"] + 1e-3 * (torch.randn(n, generator=gen, device=DEV) + 3.0))
    sg = x["g"].clone()
    sg[still & (idx % 2 == 0)] = float("inf")
    sg[still & (idx % 2 == 1)] = float("nan")
    return sg, x["p"], p, still


@pytest.mark.parametrize("n", SIZES)
def test_si_accumulate_vs_fp64(n):
    from mafed_amd import ops
    x = _inputs(n)
    sg, sp, p, still = _moved(x)
    w, w2 = x["w"].clone(), x["w"].clone()
    ops.si_accumulate_(sg, sp, p, w)
    ops.si_accumulate_(sg, sp, p, w2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(w), _bits(w2))
    assert torch.equal(_bits(w[still]), _bits(x["w"][still]))        # unmoved: bit-identical, whatever g^ holds
    assert bool(torch.isfinite(w).all())
    want, inc = si_accumulate_fp64(_np(x["w"]), _np(sg), _np(sp), _np(p))
    err, bound = np.abs(_np(w) - want), EPS22 * (np.abs(_np(x["w"])) + np.abs(inc))
    assert bool((err <= bound).all()), f"w: worst excess {float((err - bound).max()):.3e}"
    if n > 1:
        assert not torch.equal(w[~still], x["w"][~still])


@pytest.mark.parametrize("n", SIZES)
def test_si_consolidate_vs_fp64(n):
    from mafed_amd import ops
    x = _inputs(n)
    w = x["w"].clone()
    if n:
        w[::5] = -1e4            # far below -Omega (p - p*)^2 - Omega xi: the clamp gives exactly +0
    w_in, omega, anchor = w.clone(), x["omega"].clone(), x["anchor"].clone()
    ops.si_consolidate_(x["p"], anchor, w, omega, XI)
    torch.cuda.synchronize()
    assert torch.equal(_bits(anchor), _bits(x["p"])) and torch.equal(_bits(w), _bits(torch.zeros_like(w)))
    want, q = si_consolidate_fp64(_np(x["omega"]), _np(w_in), _np(x["p"]), _np(x["anchor"]), np.float32(XI))
    err, bound = np.abs(_np(omega) - want), EPS21 * (np.abs(_np(x["omega"])) + np.abs(q))
    assert bool((err <= bound).all()), f"Omega: worst excess {float((err - bound).max()):.3e}"
    if n:
        assert torch.equal(_bits(omega[::5]), _bits(torch.zeros_like(omega[::5]))) and bool((omega >= 0).all())
    if n > 1:
        assert bool((omega > 0).any())


def test_si_kernels_refuse_misaligned_buffers():
    from mafed_amd import _lib, ops
    x = _inputs(1023)
    a = {k: v.clone() for k, v in x.items()}
    nb = ops.si_blocks(1022)
    part = torch.empty(nb, device=DEV)
    with pytest.raises(_lib.MafedHipError):
        ops.si_stash(a["g"][1:], a["p"][1:], None, None, TWO_C, a["w"][1:], a["omega"][1:], part, part.clone())
    with pytest.raises(_lib.MafedHipError):
        ops.si_accumulate_(a["g"][1:], a["p"][1:], a["anchor"][1:], a["w"][1:])
    with pytest.raises(_lib.MafedHipError):
        ops.si_consolidate_(a["p"][1:], a["anchor"][1:], a["w"][1:], a["omega"][1:], XI)
    torch.cuda.synchronize()
    for k in x:
        assert torch.equal(_bits(a[k]), _bits(x[k]))


# ---- plugin level ---------------------------------------------------------------------------------------------------------------
def _model(cfg, sd, dtype=torch.float32):
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    mc = VLPythiaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        vision_hidden_size=cfg.vision_hidden_size, num_vision_tokens=cfg.num_vision_tokens)
    m = VLPythiaForCausalLM(mc, compute_dtype=dtype, device=DEV)
    m.load_state_dict(sd, strict=True)
    return m


def _to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _conf(lr=1e-3, accumulate=1, grad_norm=2.0):
    return types.SimpleNamespace(accumulate_grad_batches=accumulate, replay_interval=1, grad_norm=grad_norm, learning_rate=lr, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_steps=0, total_steps=100)


def _check_pass_b(w_before, w_after, sg, sp, p, what):
    """w's increment over one optimiser step against -g^ (p - p^) recomputed in float64, within the accumulate bound; -> the increment."""
    want, inc = si_accumulate_fp64(_np(w_before), _np(sg), _np(sp), _np(p))
    err, bound = np.abs(_np(w_after) - want), EPS22 * (np.abs(_np(w_before)) + np.abs(inc))
    assert bool((err <= bound).all()), f"{what}: w worst excess {float((err - bound).max()):.3e}"
    return inc


def test_si_task0_is_naive(monkeypatch):
    """Three Trainer steps in fp32 with grad_norm so high that the clip scale is exactly 1: loss bits and parameters equal Naive's bit
    for bit; the clip folds the stash pass's partials on task 0 too (it never reads the buffer); w equals the float64 recomputation from
    the captured (g^, p^, p) step by step."""
    from mafed_amd import SI, Naive, Trainer, ops
    from oracle import vlpythia_ref as R
    from tests.helpers import tiny_cfg
    cfg = tiny_cfg("t64")
    batches = [_to_dev(R.make_batch(cfg, 4, 6, seed=300 + i, pad=True, n_answer=3)) for i in range(3)]
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    res = {}
    for key in ("naive", "si"):
        model = _model(cfg, sd)
        method = SI(reg_lambda=256.0) if key == "si" else Naive()
        tr = Trainer(model, method, _conf(grad_norm=1e9), task_id=0)
        if key == "si":
            monkeypatch.setattr(ops, "gradnorm_clip", lambda *a, **k: pytest.fail("the clip read the gradient buffer"))
        losses = []
        for i, b in enumerate(batches):
            w0 = method.small_omega.clone() if key == "si" and method.small_omega is not None else None
            rec = tr.step(dict(b), i)
            losses.append(rec["loss"])
            if key == "si":
                assert model.final_grad_sumsq is None   # handed over and used up
                if w0 is None:
                    w0 = torch.zeros_like(method.small_omega)
                inc = _check_pass_b(w0, method.small_omega, method._stash_g, method._stash_p, model.flat_params, f"step {i}")
                assert float(np.abs(inc).max()) > 0 and float(tr.optimizer.clip_out[1]) == 1.0
                gn = float(rec["grad_norm"])
                want = float(method._stash_g.double().norm())
                assert abs(gn - want) <= 1e-6 * want
        tr.join()
        torch.cuda.synchronize()
        res[key] = (torch.stack(losses).clone(), model.flat_params.clone())
        if key == "si":
            assert float(method.last_penalty) == 0.0 and method.task_id == 0 and not bool(method.omega.any())
    assert torch.equal(_bits(res["si"][0]), _bits(res["naive"][0])), res
    assert torch.equal(_bits(res["si"][1]), _bits(res["naive"][1]))


def _si_run(cls, c, dtype=torch.float32, overwrite=True, pipeline=False, checks=False):
    """SI_TRAINER through Trainer.step with plugin class ``cls``.  ``checks`` (bf16 test): per optimiser step, w's increment after
    tr.join() against float64, and on the last step the gradient of layer 0's weight matrices just before the clip against
    g^ + 2c Omega (p^ - p*)."""
    from mafed_amd import Trainer
    k = SI_TRAINER
    cfg, sd, _, batches = trainer_case()
    model = _model(cfg, sd, dtype)
    if dtype == torch.bfloat16:
        model.dw_group_layers = 2
    si = cls(reg_lambda=c, xi=k["xi"], opts=types.SimpleNamespace(accumulate_grad_batches=k["accumulate"]))
    tr = Trainer(model, si, _conf(lr=k["lr"], accumulate=k["accumulate"], grad_norm=k["grad_clip"]), task_id=0,
                 overwrite_weight_grads=overwrite, pipeline_optimizer=pipeline)
    assert tr._overwrite_ok() == (overwrite and dtype == torch.bfloat16)
    captured = {}
    if checks:
        lo, hi = model.layer_matrix_range(0)
        clip = tr.optimizer.clip_grad_norm_

        def clip_and_capture(*a, **kws):
            captured["g"] = model.flat_grads[lo:hi].clone()
            return clip(*a, **kws)
        tr.optimizer.clip_grad_norm_ = clip_and_capture
    losses, gns, pens = [], [], []
    for i in range(k["n_micro"]):
        if i == k["update_after"]:
            tr.join()
            si.update(model)
        w0 = si.small_omega.clone() if checks and si.small_omega is not None else None
        rec = tr.step(_to_dev(batches[i][0]), i)
        assert rec["branch"] == "task" and torch.is_tensor(rec["loss"]) and rec["loss"].is_cuda
        losses.append(rec["loss"])
        if not rec["stepped"]:
            continue
        gns.append(rec["grad_norm"])
        pens.append(si.last_penalty.clone() if si.last_penalty is not None else torch.zeros((), device=DEV))
        if checks:
            tr.join()
            w1 = si.small_omega
            if w0 is None:
                w0 = torch.zeros_like(w1)
            inc = _check_pass_b(w0, w1, si._stash_g, si._stash_p, model.flat_params, f"micro-batch {i}")
            assert float((np.abs(inc) > 0).mean()) > 0.5, "the optimiser moved less than half of the parameters"
            if si.task_id > 0 and i == k["n_micro"] - 1:
                sl = slice(lo, hi)
                want, term, _ = si_stash_fp64(_np(si._stash_g[sl]), _np(si._stash_p[sl]), _np(si.omega[sl]), _np(si.anchor[sl]), np.float32(2.0 * c))
                err, bound = np.abs(_np(captured["g"]) - want), EPS22 * (np.abs(_np(si._stash_g[sl])) + np.abs(term))
                assert float(np.abs(term).max()) > 0 and float(np.abs(_np(si._stash_g[sl])).max()) > 0
                assert bool((err <= bound).all()), f"weight-matrix gradient in front of the clip: worst excess {float((err - bound).max()):.3e}"
                captured["term_over_g"] = float(np.linalg.norm(term) / np.linalg.norm(_np(si._stash_g[sl])))
    tr.join()
    torch.cuda.synchronize()
    f = lambda xs: [float(x) for x in xs]
    return dict(loss=f(losses), gn=f(gns), pen=f(pens), params=model.flat_params.clone(), model=model, si=si, captured=captured)


def _views(model, flat):
    from mafed_amd.methods.flat import FlatDict
    return FlatDict(model, flat)


def test_si_trainer_matches_torch_double():
    """Four optimiser steps at accumulate = 2, fp32: two of task 0, update(model), two of task 1, against a twin Trainer whose plugin
    does the same hooks with torch ops in float64.  Micro-batches 0 .. 7 of tests.helpers.trainer_case() (task-batch seeds 33 .. 40),
    c = 256, xi = 1e-3.  Along the float64 oracle's trajectory (tests/si_ref.py::si_trainer_fp64, checked on the CPU by
    tests/test_si_ref.py::test_trainer_case_conditions) the penalty gradient is zero on steps 0 .. 2 and on step 3 has norm 2.0859
    against a task gradient of 3.7864 (ratio 0.551), the penalty is 0.28343, 91.8 % of the parameters have Omega > 0, and the run with
    c = 0 ends 4.9e-4 away in the parameters."""
    from mafed_amd import SI
    c = SI_TRAINER["c"]
    a = _si_run(SI, c)
    b = _si_run(make_torch_si(), c)
    z = _si_run(SI, 0.0)
    print(f"[si] trainer: grad norms {a['gn']} / twin {b['gn']}, penalties {a['pen']} / twin {b['pen']}")
    assert len(a["loss"]) == 8 and len(a["gn"]) == 4 and a["si"].task_id == 1 and b["si"].task_id == 1
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert abs(x - y) <= 1e-6 * abs(y), f"micro-batch {i}: loss {x} vs {y}"
    for i, (x, y) in enumerate(zip(a["gn"], b["gn"])):
        assert abs(x - y) <= 1e-5 * abs(y), f"step {i}: grad norm {x} vs {y}"
    d = float((a["params"] - b["params"]).abs().max())
    print(f"[si] trainer: parameters differ by {d:.3e} after 4 optimiser steps")
    assert d <= 1e-6, f"parameters differ by {d} after 4 optimiser steps"
    for which in ("small_omega", "omega", "anchor"):
        got, ref = a["si"].named(a["model"], which), _views(b["model"], getattr(b["si"], which))
        for name in ref:
            assert_rel_close(got[name], ref[name], TOL, f"{which} {name}")
    assert a["pen"][:3] == [0.0, 0.0, 0.0] and abs(a["pen"][3] - b["pen"][3]) <= 1e-5 * b["pen"][3]
    ref = si_trainer_fp64()
    assert abs(a["pen"][3] - ref["steps"][3]["penalty"]) <= TOL * ref["steps"][3]["penalty"]
    assert float((a["si"].omega > 0).float().mean()) >= 0.10
    # the case can see the penalty
    dz = float((a["params"] - z["params"]).abs().max())
    print(f"[si] trainer: c = {c} against c = 0: parameters differ by {dz:.3e}")
    assert dz > 100 * 1e-6


def test_si_bf16_default_trainer_pipelined():
    """bf16 with the Trainer's defaults (overwriting first sweep, ``dw_group_layers = 2``) and the pipelined optimiser.  The window's
    first sweep overwrites the weight-matrix gradients, and the penalty gradient still arrives: on layer 0's matrices the gradient in
    front of the clip is g^ + 2c Omega (p^ - p*) within the kernel bound.  After tr.join() w has moved by -g^ (p - p^) on every step --
    a pass B that ran ahead of the optimiser would have left it where it was.  Overwrite on against off: the bounds of
    tests/test_gpu_agem.py::test_agem_bf16_overwrite_mode_equals_zero_then_accumulate."""
    from mafed_amd import SI
    c = SI_TRAINER["c"]
    a = _si_run(SI, c, torch.bfloat16, overwrite=True, pipeline=True, checks=True)
    b = _si_run(SI, c, torch.bfloat16, overwrite=False, pipeline=True, checks=True)
    print(f"[si] bf16: penalties {a['pen']} / {b['pen']}, |term| / |g^| on layer 0's matrices {a['captured']['term_over_g']:.3f}")
    assert a["pen"][3] > 0 and a["captured"]["term_over_g"] > 0.01
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), f"micro-batch {i}: loss {x} vs {y}"
    assert len(a["gn"]) == 4
    for i, (x, y) in enumerate(zip(a["gn"], b["gn"])):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), f"step {i}: grad norm {x} vs {y}"
    d = float((a["params"] - b["params"]).abs().max())
    assert d <= 2e-5, f"parameters differ by {d} after 4 optimiser steps"
    assert a["model"]._dw_stale and not b["model"]._dw_stale


def test_si_skipped_step_leaves_no_trace():
    """One inf planted in flat_grads in front of the hook, on task 1 with w and Omega non-zero: the norm is not finite, the clip scale
    is -1, the step is skipped -- parameters and w bit-unchanged although g^ holds the inf."""
    from mafed_amd import SI, Trainer
    cfg, sd, _, batch, _ = golden_setup("t64")
    model = _model(cfg, sd)
    si = SI(reg_lambda=4.0)
    tr = Trainer(model, si, _conf(), task_id=0)
    tr.step(_to_dev(batch), 0)
    si.update(model)
    tr.step(_to_dev(batch), 1)
    assert si.task_id == 1 and bool(si.omega.any()) and bool(si.small_omega.any())
    w0, p0 = si.small_omega.clone(), model.flat_params.clone()
    hook = si.update_after_backward

    def poisoned(model=None, **kw):
        model.flat_grads[5] = float("inf")
        hook(model=model, **kw)
    si.update_after_backward = poisoned
    rec = tr.step(_to_dev(batch), 2)
    torch.cuda.synchronize()
    assert rec["stepped"] and not np.isfinite(float(rec["grad_norm"])) and float(tr.optimizer.clip_out[1]) == -1.0
    assert not bool(torch.isfinite(si._stash_g).all())
    assert torch.equal(_bits(model.flat_params), _bits(p0)) and torch.equal(_bits(si.small_omega), _bits(w0))
    # and the next, clean step moves both again
    si.update_after_backward = hook
    tr.step(_to_dev(batch), 3)
    torch.cuda.synchronize()
    assert not torch.equal(model.flat_params, p0) and not torch.equal(si.small_omega, w0) and bool(torch.isfinite(si.small_omega).all())


def test_si_refusals():
    from mafed_amd import SI, Trainer
    cfg, sd, _, batch, _ = golden_setup("t64")
    model = _model(cfg, sd)
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, SI(), _conf(), reducer=types.SimpleNamespace(world=2))   # a stub: refused before anything looks at it
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, SI(), _conf(), ddp=True)
    Trainer(model, SI(), _conf())
    foreign = torch.nn.Linear(2, 2).to(DEV)
    si = SI()
    for call in (lambda: si.update(foreign), lambda: si.update_after_backward(model=foreign), lambda: si.update_after_step(model=foreign)):
        with pytest.raises(TypeError, match="native model"):
            call()
