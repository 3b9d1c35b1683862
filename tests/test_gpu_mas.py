"""Memory Aware Synapses (mafed_amd/methods/mas.py, csrc/mas.hip, csrc/sqnorm.hip): the three flat-buffer passes and the two head kernels
against float64 numpy, the importance pass against the oracle model under autograd, and the plugin's life inside Trainer.step -- task 0
against Naive, a task boundary against a float64 torch twin, the bf16 default Trainer with the pipelined optimiser, the checkpoint round
trip and the refusals."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import assert_rel_close, golden_setup, trainer_case
from tests.mas_ref import (MAS_TRAINER, make_torch_mas, mas_accumulate_fp64, mas_consolidate_fp64, mas_importances_fp64, mas_loader,
                           mas_penalty_fp64, mas_trainer_fp64, sqnorm_fp64)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3   # the project's fp32 gate
EPS23, EPS22 = 2.0 ** -23, 2.0 ** -22

# the sizes of tests/test_gpu_si.py: 0: empty; 1, 3: tail only; 4: one vector; 1023: less than one block; 4 * 1024 + 1: several blocks and
# a tail behind full vectors; 3 * 2^21 + 5: above 2 * 2048 * 256 * 4, so the grid-stride loop at the grid cap goes through its
# two-accumulator body and on
SIZES = [0, 1, 3, 4, 1023, 4 * 1024 + 1, 3 * 2 ** 21 + 5]
TWO_C, WEIGHT, SEEN, ALPHA = 1.5, 3.0, 5, 0.25   # (alpha is exact in fp32; 1 / SEEN is not, and its rounding is one of the counted ones)

_INPUTS = {}


def _inputs(n):
    """{g, p, omega, anchor, acc} fp32 on the device; built once per size and left unchanged.  g carries a -0.0."""
    if n not in _INPUTS:
        gen = torch.Generator().manual_seed(3000 + n % 997)
        g, p = (torch.randn(n, generator=gen) for _ in range(2))
        if n > 2:
            g[2] = -0.0
        anchor = p + 0.05 * torch.randn(n, generator=gen)
        omega, acc = (torch.randn(n, generator=gen).abs() for _ in range(2))
        _INPUTS[n] = {k: v.to(DEV) for k, v in dict(g=g, p=p, omega=omega, anchor=anchor, acc=acc).items()}
    return _INPUTS[n]


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.int32)


def _np(t):
    return t.double().cpu().numpy()


# ---- flat passes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_mas_accumulate_vs_fp64(n):
    """acc' = fma(w, |g|, acc): two roundings at most (the product is exact inside the fma: one), bound 2^-23 (|acc| + w |g|)."""
    from mafed_amd import ops
    x = _inputs(n)
    a, b, neg = x["acc"].clone(), x["acc"].clone(), x["acc"].clone()
    ops.mas_accumulate_(x["g"], a, WEIGHT)
    ops.mas_accumulate_(x["g"], b, WEIGHT)
    ops.mas_accumulate_(-x["g"], neg, WEIGHT)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))        # run to run
    assert torch.equal(_bits(a), _bits(neg))      # Omega does not see the sign of g
    want, inc = mas_accumulate_fp64(_np(x["acc"]), _np(x["g"]), WEIGHT)
    err, bound = np.abs(_np(a) - want), EPS23 * (np.abs(_np(x["acc"])) + inc)
    assert bool((err <= bound).all()), f"acc: worst excess {float((err - bound).max()):.3e}"
    if n > 2:
        assert torch.equal(_bits(a[2]), _bits(x["acc"][2]))   # the -0.0 adds nothing
        assert bool((a >= x["acc"]).all()) and not torch.equal(a, x["acc"])


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("n", SIZES)
def test_mas_consolidate_vs_fp64(n, first):
    """Omega' within 2^-22 (alpha |Omega| + (1 - alpha) |acc / N|) (three roundings on the new term, one on the old: DESIGN 4k), anchor
    == p and acc == 0 bit for bit.  On the first task Omega is not read: it holds NaN here."""
    from mafed_amd import ops
    x = _inputs(n)
    acc, anchor = x["acc"].clone(), x["anchor"].clone()
    omega = torch.full_like(x["omega"], float("nan")) if first else x["omega"].clone()
    ops.mas_consolidate_(acc, omega, x["p"], anchor, 1.0 / SEEN, ALPHA, first)
    torch.cuda.synchronize()
    assert torch.equal(_bits(anchor), _bits(x["p"])) and torch.equal(_bits(acc), _bits(torch.zeros_like(acc)))
    want, old, new = mas_consolidate_fp64(_np(x["omega"]), _np(x["acc"]), SEEN, ALPHA, first)
    err, bound = np.abs(_np(omega) - want), EPS22 * (np.abs(old) + np.abs(new))
    assert bool((err <= bound).all()), f"Omega: worst excess {float((err - bound).max()):.3e}"
    if n:   # (|randn| of 6 M draws holds an exact zero or two)
        assert bool((omega >= 0).all()) and bool((omega > 0).any())


def _penalty(x):
    from mafed_amd import ops
    n = x["g"].numel()
    g = x["g"].clone()
    nb = ops.mas_blocks(n)
    sumsq, pen = torch.full((nb + 3,), -7.0, device=DEV), torch.full((nb + 3,), -7.0, device=DEV)
    ops.mas_penalty_(g, x["p"], x["omega"], x["anchor"], TWO_C, sumsq, pen)
    return g, sumsq, pen, nb


@pytest.mark.parametrize("n", SIZES)
def test_mas_penalty_vs_fp64(n):
    from mafed_amd import ops
    x = _inputs(n)
    g, sumsq, pen, nb = _penalty(x)
    again = _penalty(x)
    torch.cuda.synchronize()
    for a, b in zip((g, sumsq, pen), again):   # run to run: the same bits
        assert torch.equal(_bits(a), _bits(b))
    assert nb == ops.si_blocks(n) and 1 <= nb <= 2048 and bool((sumsq[nb:] == -7.0).all()) and bool((pen[nb:] == -7.0).all())
    want, term, pen64 = mas_penalty_fp64(_np(x["g"]), _np(x["p"]), _np(x["omega"]), _np(x["anchor"]), TWO_C)
    err, bound = np.abs(_np(g) - want), EPS22 * (np.abs(_np(x["g"])) + np.abs(term))
    assert bool((err <= bound).all()), f"g': worst excess {float((err - bound).max()):.3e}"
    if n:
        assert not torch.equal(g, x["g"])
    # one copy of the arithmetic: SI's stash pass with the same inputs leaves the same g' and the same partials
    g_si, sq_si, pen_si = x["g"].clone(), torch.empty(nb, device=DEV), torch.empty(nb, device=DEV)
    ops.si_stash(g_si, x["p"], x["omega"], x["anchor"], TWO_C, torch.empty_like(g_si), torch.empty_like(g_si), sq_si, pen_si)
    assert torch.equal(_bits(g), _bits(g_si)) and torch.equal(_bits(sumsq[:nb]), _bits(sq_si)) and torch.equal(_bits(pen[:nb]), _bits(pen_si))
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
    c = TWO_C / 2
    got = float(ops.si_penalty_finish(pen[:nb], c))
    print(f"[mas] n {n}: norm {float(folded[0]):.8g} (fp64 {ref64:.8g}), penalty {got:.8g} (fp64 {c * pen64:.8g})")
    assert abs(got - c * pen64) <= 1e-5 * c * pen64
    if n == 0:
        assert got == 0.0


def test_mas_kernels_refuse_misaligned_buffers():
    from mafed_amd import _lib, ops
    x = _inputs(1023)
    a = {k: v.clone() for k, v in x.items()}
    part = torch.empty(ops.mas_blocks(1022), device=DEV)
    with pytest.raises(_lib.MafedHipError):
        ops.mas_accumulate_(a["g"][1:], a["acc"][1:], WEIGHT)
    with pytest.raises(_lib.MafedHipError):
        ops.mas_consolidate_(a["acc"][1:], a["omega"][1:], a["p"][1:], a["anchor"][1:], 1.0 / SEEN, ALPHA, False)
    with pytest.raises(_lib.MafedHipError):
        ops.mas_penalty_(a["g"][1:], a["p"][1:], a["omega"][1:], a["anchor"][1:], TWO_C, part, part.clone())
    torch.cuda.synchronize()
    for k in x:
        assert torch.equal(_bits(a[k]), _bits(x[k]))


# ---- head kernels ---------------------------------------------------------------------------------------------------------------
def _head_inputs(B, T, V, dtype):
    """Logits (scale 3) and labels: the last sample has no labelled row; sample 0 has a label in the last position (the shift hands it to
    row T - 2; the last row is never labelled) and one in position 0 (the shift drops it)."""
    gen = torch.Generator().manual_seed(B * 1000 + T * 100 + V % 97)
    z = (3.0 * torch.randn(B, T, V, generator=gen)).to(dtype)
    lab = torch.full((B, T), -100, dtype=torch.int64)
    lab[0, 0], lab[0, 1], lab[0, T - 1] = 1, V - 1, 2
    if B > 2:
        lab[1, 1:T - 1] = torch.arange(T - 2) % V
    return z.to(DEV), lab.to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,T,V", [(3, 5, 4), (3, 5, 1028), (2, 3, 50304)])
def test_sqnorm_kernels_vs_fp64(B, T, V, dtype):
    """rowsq and J at 1e-5 relative; dlogits within one rounding of the output dtype on top of the fp32 product (2^-8 relative in bf16,
    2^-23 in fp32: the scale 2 dloss / (B count) and the product are one fp32 rounding each); exact zeros on unlabelled rows, which
    the kernel writes (the output buffer starts as NaN); a raised poison flag gives NaN."""
    from mafed_amd import ops
    z, lab = _head_inputs(B, T, V, dtype)
    dloss = torch.tensor([0.75], device=DEV)
    J, rowsq = ops.sqnorm_fwd(z, lab)
    J2, rowsq2 = ops.sqnorm_fwd(z, lab, poison=torch.zeros(1, dtype=torch.int32, device=DEV))
    Jp, _ = ops.sqnorm_fwd(z, lab, poison=torch.ones(1, dtype=torch.int32, device=DEV))
    dz = ops.sqnorm_bwd(z, lab, dloss, out=torch.full_like(z, float("nan")))
    dz2 = ops.sqnorm_bwd(z, lab, dloss)
    torch.cuda.synchronize()
    assert torch.equal(_bits(J), _bits(J2)) and torch.equal(_bits(rowsq), _bits(rowsq2)) and torch.equal(dz.view(torch.uint8), dz2.view(torch.uint8))
    assert bool(torch.isnan(Jp).all())
    want_rowsq, want_J, want_dz = sqnorm_fp64(_np(z), lab.cpu().numpy(), dloss=0.75)
    labelled = want_rowsq != 0
    assert labelled.sum() == (T if B > 2 else 2) and not labelled[-1].any() and not labelled[:, -1].any() and labelled[0, T - 2]
    got_rowsq = _np(rowsq)
    assert bool((np.abs(got_rowsq - want_rowsq) <= 1e-5 * want_rowsq).all()), (got_rowsq, want_rowsq)
    assert bool((got_rowsq[~labelled] == 0.0).all())
    print(f"[mas] sqnorm {B}x{T}x{V} {dtype}: J {float(J):.8g} (fp64 {want_J:.8g})")
    assert abs(float(J) - want_J) <= 1e-5 * want_J
    got = _np(dz)
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23
    err = np.abs(got - want_dz)
    assert bool((err <= eps * np.abs(want_dz)).all()), f"dlogits: worst excess {float((err - eps * np.abs(want_dz)).max()):.3e}"
    assert bool((got[~labelled] == 0.0).all()) and bool((got[labelled] != 0.0).any())
    assert dz.dtype == dtype


def _ragged_batch(cfg, B, T, n_ans, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g)
    am = torch.ones(B, T, dtype=torch.int64)
    labels = torch.full((B, T), -100, dtype=torch.int64)
    for b in range(B):
        k = int(torch.randint(0, n_ans + 1, (1,), generator=g))
        if k:
            labels[b, -k:] = ids[b, -k:]
        am[b, :int(torch.randint(0, 3, (1,), generator=g))] = 0
    feats = torch.randn(B, cfg.num_vision_tokens, cfg.vision_hidden_size, generator=g)
    return {"input_ids": ids.to(DEV), "attention_mask": am.to(DEV), "labels": labels.to(DEV), "patch_embeddings": feats.to(DEV)}


@pytest.mark.parametrize("dtype,B,T,n_ans", [(torch.float32, 6, 12, 3), (torch.bfloat16, 32, 16, 3)])
def test_sparse_head_equals_dense_head_under_sqnorm(dtype, B, T, n_ans, monkeypatch):
    """The same batch with and without ``max_label_rows`` under ``head_loss = SquaredNorm()``: equal J and gradients (the shapes and
    bounds of tests/test_gpu_lwf.py::test_sparse_head_equals_dense_head_with_a_logit_teacher), the sparse run on the B * Rc compact rows;
    the cross-entropy kernels are not called.  Then ``MAS.update`` on the model with LwF installed: its teacher and the CE + KL kernels are
    not called during the importance pass, and LwF's object is back in the slot afterwards."""
    from mafed_amd import CLMethod, MAS, VLPythiaConfig, VLPythiaForCausalLM, ops
    from mafed_amd.head_loss import LogitDistillation, SquaredNorm
    cfg = VLPythiaConfig(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                         vision_hidden_size=32, num_vision_tokens=8)
    model = VLPythiaForCausalLM(cfg, compute_dtype=dtype, device=DEV, seed=5)
    batch = _ragged_batch(cfg, B, T, n_ans, seed=B + T)
    shapes, fwd = [], ops.sqnorm_fwd

    def spy(logits, labels, poison=None):
        shapes.append((tuple(logits.shape), tuple(labels.shape), poison is not None))
        return fwd(logits, labels, poison=poison)
    monkeypatch.setattr(ops, "sqnorm_fwd", spy)
    for name in ("ce_fwd", "ce_bwd", "ce_kd_fwd", "ce_kd_bwd"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} ran under the squared-norm head loss"))
    model.head_loss = SquaredNorm()

    def run(hint):
        model.zero_grad()
        kw = {"max_label_rows": hint} if hint is not None else {}
        out = model(**batch, **kw, return_dict=True)
        out.loss.backward()
        torch.cuda.synchronize()
        return float(out.loss.detach()), model.flat_grads.clone()

    l0, g0 = run(None)
    l1, g1 = run(n_ans)
    assert int(model.last_label_overflow) == 0 and l0 > 0
    Rc = n_ans + 1 if dtype == torch.float32 else next(r for r in range(n_ans + 1, T + 1) if (B * r) % 128 == 0)
    V = cfg.vocab_size
    assert shapes == [((B, T, V), (B, T), False), ((B, Rc, V), (B, Rc), True)] and Rc < T, shapes
    tol = 1e-6 if dtype == torch.float32 else 2e-3
    assert abs(l1 - l0) <= tol * max(1.0, abs(l0)), (l0, l1)
    rel = float((g1 - g0).norm() / g0.norm())
    print(f"[mas] sparse vs dense head, {dtype}: J {l0} / {l1}, gradient relative difference {rel:.3e}")
    assert rel <= (1e-5 if dtype == torch.float32 else 1e-2), f"gradients: relative difference {rel:.3e}"
    # the teacher does not run in the importance pass (ce_kd_fwd / ce_kd_bwd still fail the test if called)
    model.head_loss = None
    lwf = CLMethod["lwf"]()
    lwf.update(model)
    installed = model.head_loss
    assert isinstance(installed, LogitDistillation)
    installed.teacher = lambda *a, **k: pytest.fail("the logit teacher ran in the MAS importance pass")
    mas = MAS()
    mas.update(model, dataloader=[batch])
    torch.cuda.synchronize()
    assert mas.task_id == 1 and model.head_loss is installed and len(shapes) == 3


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


def test_mas_importance_pass_matches_oracle_autograd():
    """Omega_new from compute_importances on the golden t64 model in fp32, over the golden batch (3 samples) and the first 2 samples of a
    second one, per parameter tensor against the oracle model under autograd in float64 with the same objective.  Around the pass:
    ``head_loss`` is empty again, also when a batch raises, the gradient buffer is zero, and a forward under the default objective
    gives the same bits for logits and loss as before."""
    from mafed_amd import MAS
    from oracle import vlpythia_ref as R
    cfg, sd, _, batch, _ = golden_setup("t64")
    second = R.make_batch(cfg, 3, 6, seed=91, pad=True, n_answer=3)
    loader = [batch, {k: v[:2].clone() for k, v in second.items()}]
    model = _model(cfg, sd)

    def probe():
        with torch.no_grad():
            out = model(**_to_dev(batch), return_dict=True)
        return out.loss.clone(), out.logits.clone()

    loss0, logits0 = probe()
    mas = MAS()
    got = mas.compute_importances(model, [_to_dev(b) for b in loader])
    torch.cuda.synchronize()
    assert model.head_loss is None and not bool(model.flat_grads.any()) and mas.omega is None and mas.task_id == 0
    loss1, logits1 = probe()
    assert torch.equal(_bits(loss0), _bits(loss1)) and torch.equal(_bits(logits0), _bits(logits1))
    ref = mas_importances_fp64(cfg, sd, loader)
    assert set(got) == set(ref)
    for name in ref:
        assert_rel_close(got[name], ref[name], TOL, f"Omega {name}")
        assert bool((got[name] >= 0).all())
    assert float(got["embed_out.weight"].max()) > 0

    def broken():
        yield _to_dev(batch)
        raise RuntimeError("loader failed")
    with pytest.raises(RuntimeError, match="loader failed"):
        mas.compute_importances(model, broken())
    assert model.head_loss is None and not bool(model.flat_grads.any())
    with pytest.raises(ValueError, match="empty"):
        mas.compute_importances(model, [])


def test_mas_task0_is_naive():
    """Three Trainer steps in fp32 with grad_norm so high that the clip scale is exactly 1 (as tests/test_gpu_si.py does): loss bits and
    parameters equal Naive's bit for bit; the plugin holds no state and hands no norm over."""
    from mafed_amd import MAS, Naive, Trainer
    from oracle import vlpythia_ref as R
    from tests.helpers import tiny_cfg
    cfg = tiny_cfg("t64")
    batches = [_to_dev(R.make_batch(cfg, 4, 6, seed=300 + i, pad=True, n_answer=3)) for i in range(3)]
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    res = {}
    for key in ("naive", "mas"):
        model = _model(cfg, sd)
        method = MAS(reg_lambda=256.0) if key == "mas" else Naive()
        tr = Trainer(model, method, _conf(grad_norm=1e9), task_id=0)
        losses = []
        for i, b in enumerate(batches):
            rec = tr.step(dict(b), i)
            losses.append(rec["loss"])
            assert model.final_grad_sumsq is None and float(tr.optimizer.clip_out[1]) == 1.0
        tr.join()
        torch.cuda.synchronize()
        res[key] = (torch.stack(losses).clone(), model.flat_params.clone())
        if key == "mas":
            assert method.omega is None and method.last_penalty is None and method.task_id == 0
    assert torch.equal(_bits(res["mas"][0]), _bits(res["naive"][0])), res
    assert torch.equal(_bits(res["mas"][1]), _bits(res["naive"][1]))


def _mas_run(cls, c, dtype=torch.float32, overwrite=True, pipeline=False, checks=False):
    """MAS_TRAINER through Trainer.step with plugin class ``cls``.  ``checks`` (bf16 test): on every step of task 1 the gradient of layer
    0's weight matrices just before the clip against g^ + 2c Omega (p - p*), g^ and p captured in front of the hook."""
    from mafed_amd import Trainer
    k = MAS_TRAINER
    cfg, sd, _, batches = trainer_case()
    model = _model(cfg, sd, dtype)
    init = model.flat_params.clone()
    if dtype == torch.bfloat16:
        model.dw_group_layers = 2
    mas = cls(reg_lambda=c, alpha=k["alpha"], opts=types.SimpleNamespace(accumulate_grad_batches=k["accumulate"]))
    tr = Trainer(model, mas, _conf(lr=k["lr"], accumulate=k["accumulate"], grad_norm=k["grad_clip"]), task_id=0,
                 overwrite_weight_grads=overwrite, pipeline_optimizer=pipeline)
    assert tr._overwrite_ok() == (overwrite and dtype == torch.bfloat16)
    captured = {"term_over_g": []}
    if checks:
        lo, hi = model.layer_matrix_range(0)
        sl = slice(lo, hi)
        clip, hook = tr.optimizer.clip_grad_norm_, mas.update_after_backward

        def hook_and_capture(model=None, **kws):
            captured["g_hat"], captured["p_hat"] = model.flat_grads[sl].clone(), model.flat_params[sl].clone()
            return hook(model=model, **kws)

        def clip_and_capture(*a, **kws):
            captured["g"] = model.flat_grads[sl].clone()
            return clip(*a, **kws)
        mas.update_after_backward, tr.optimizer.clip_grad_norm_ = hook_and_capture, clip_and_capture
    losses, gns, pens = [], [], []
    for i in range(k["n_micro"]):
        if i == k["update_after"]:
            tr.join()
            mas.update(model, dataloader=[_to_dev(b) for b in mas_loader(batches)])
            assert model.head_loss is None
        rec = tr.step(_to_dev(batches[i][0]), i)
        assert rec["branch"] == "task" and rec["stepped"] and torch.is_tensor(rec["loss"]) and rec["loss"].is_cuda
        losses.append(rec["loss"])
        gns.append(rec["grad_norm"])
        pens.append(mas.last_penalty.clone() if mas.last_penalty is not None else torch.zeros((), device=DEV))
        if checks and mas.task_id > 0:
            g_hat = _np(captured["g_hat"])
            want, term, _ = mas_penalty_fp64(g_hat, _np(captured["p_hat"]), _np(mas.omega[sl]), _np(mas.anchor[sl]), np.float32(2.0 * c))
            err, bound = np.abs(_np(captured["g"]) - want), EPS22 * (np.abs(g_hat) + np.abs(term))
            assert float(np.abs(g_hat).max()) > 0
            assert bool((err <= bound).all()), f"micro-batch {i}: weight-matrix gradient in front of the clip: worst excess {float((err - bound).max()):.3e}"
            captured["term_over_g"].append(float(np.linalg.norm(term) / np.linalg.norm(g_hat)))
    tr.join()
    torch.cuda.synchronize()
    f = lambda xs: [float(x) for x in xs]
    return dict(loss=f(losses), gn=f(gns), pen=f(pens), params=model.flat_params.clone(), init=init, model=model, mas=mas, captured=captured)


def test_mas_trainer_matches_torch_double():
    """Six optimiser steps in fp32: three of task 0, update(model, loader), three of task 1, against a twin Trainer whose plugin does the
    same hooks with torch ops in float64.  Micro-batches 0 .. 5 of tests.helpers.trainer_case(), the importance loader of
    tests/mas_ref.py::mas_loader (sizes 3 and 2), c = 4, alpha = 0.5.  Along the float64 oracle's trajectory (mas_trainer_fp64, checked
    on the CPU by tests/test_mas_ref.py::test_trainer_case_conditions) the penalty gradient is zero on steps 0 .. 3 (on step 3 p = p*)
    and on step 5 has norm 1.248 against a task gradient of 4.358 (ratio 0.29), the penalty is 0.2164 and 91.5 % of the parameters have
    Omega > 0."""
    from mafed_amd import MAS
    from mafed_amd.methods.flat import FlatDict
    c = MAS_TRAINER["c"]
    a = _mas_run(MAS, c)
    b = _mas_run(make_torch_mas(), c)
    z = _mas_run(MAS, 0.0)
    print(f"[mas] trainer: grad norms {a['gn']} / twin {b['gn']}, penalties {a['pen']} / twin {b['pen']}")
    assert len(a["loss"]) == 6 and len(a["gn"]) == 6 and a["mas"].task_id == 1 and b["mas"].task_id == 1
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert abs(x - y) <= TOL * abs(y), f"micro-batch {i}: loss {x} vs {y}"
    for i, (x, y) in enumerate(zip(a["gn"], b["gn"])):
        assert abs(x - y) <= TOL * abs(y), f"step {i}: grad norm {x} vs {y}"
    for which in ("omega", "anchor"):
        got, ref = a["mas"].named(a["model"], which), FlatDict(b["model"], getattr(b["mas"], which))
        for name in ref:
            assert_rel_close(got[name], ref[name], TOL, f"{which} {name}")
    ga, gb = FlatDict(a["model"], a["params"] - a["init"]), FlatDict(b["model"], b["params"] - b["init"])
    for name in gb:
        assert_rel_close(ga[name], gb[name], TOL, f"update {name}")
    assert a["pen"][:4] == [0.0, 0.0, 0.0, 0.0] and a["pen"][4] > 0
    for i in (4, 5):
        assert abs(a["pen"][i] - b["pen"][i]) <= TOL * b["pen"][i], (i, a["pen"], b["pen"])
    ref = mas_trainer_fp64()
    assert abs(a["pen"][5] - ref["steps"][5]["penalty"]) <= TOL * ref["steps"][5]["penalty"]
    assert float((a["mas"].omega > 0).float().mean()) >= 0.5
    # the case can see the penalty
    dz = float((a["params"] - z["params"]).abs().max())
    print(f"[mas] trainer: c = {c} against c = 0: parameters differ by {dz:.3e}")
    assert dz > 100 * 1e-6


def test_mas_bf16_default_trainer_pipelined():
    """bf16 with the Trainer's defaults (overwriting first sweep, ``dw_group_layers = 2``) and the pipelined optimiser.  The window's
    first sweep overwrites the weight-matrix gradients, and the penalty gradient still arrives: on layer 0's matrices the gradient in
    front of the clip is g^ + 2c Omega (p - p*) within the kernel bound, on every step of task 1.  Overwrite on against off: the bounds of
    tests/test_gpu_si.py::test_si_bf16_default_trainer_pipelined."""
    from mafed_amd import MAS
    c = MAS_TRAINER["c"]
    a = _mas_run(MAS, c, torch.bfloat16, overwrite=True, pipeline=True, checks=True)
    b = _mas_run(MAS, c, torch.bfloat16, overwrite=False, pipeline=True, checks=True)
    print(f"[mas] bf16: penalties {a['pen']} / {b['pen']}, |term| / |g^| on layer 0's matrices {a['captured']['term_over_g']}")
    assert a["pen"][5] > 0 and len(a["captured"]["term_over_g"]) == 3 and a["captured"]["term_over_g"][0] == 0.0 and a["captured"]["term_over_g"][2] > 0.01
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), f"micro-batch {i}: loss {x} vs {y}"
    for i, (x, y) in enumerate(zip(a["gn"], b["gn"])):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), f"step {i}: grad norm {x} vs {y}"
    d = float((a["params"] - b["params"]).abs().max())
    assert d <= 2e-5, f"parameters differ by {d} after 6 optimiser steps"
    assert a["model"]._dw_stale and not b["model"]._dw_stale


def test_mas_state_dict_round_trip():
    """{omega, anchor, task_id} and nothing else; a plugin restored from it takes the same step, bit for bit."""
    from mafed_amd import MAS, Trainer
    cfg, sd, _, batch, _ = golden_setup("t64")
    dev = _to_dev(batch)
    models = [_model(cfg, sd), _model(cfg, sd)]
    first = MAS(reg_lambda=4.0)
    assert first.state_dict() == {"omega": None, "anchor": None, "task_id": 0}
    tr = Trainer(models[0], first, _conf(), task_id=0)
    tr.step(dict(dev), 0)
    first.update(models[0], dataloader=[dev])
    first.update(models[0], dataloader=[dev])   # a later task: alpha Omega + (1 - alpha) Omega_new
    state = first.state_dict()
    assert set(state) == {"omega", "anchor", "task_id"} and state["task_id"] == 2 and bool((state["omega"] > 0).any())
    assert torch.equal(state["anchor"], models[0].flat_params)
    second = MAS(reg_lambda=4.0)
    second.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in state.items()})
    assert second.task_id == 2
    with pytest.raises(ValueError, match="anchor"):
        MAS().load_state_dict({"omega": state["omega"], "task_id": 1})
    models[1].load_state_dict(models[0].state_dict(), strict=True)
    # the penalised gradient of one backward at parameters moved away from the anchor, from either plugin
    grads = []
    for plugin, m in ((first, models[0]), (second, models[1])):
        with torch.no_grad():
            m.flat_params.add_(0.01)
        m._shadow_dirty = True
        m.zero_grad()
        m(**dev, return_dict=True).loss.backward()
        plugin.update_after_backward(model=m)
        grads.append((m.flat_grads.clone(), plugin.last_penalty.clone(), m.final_grad_sumsq.clone()))
    torch.cuda.synchronize()
    for x, y in zip(*grads):
        assert torch.equal(_bits(x), _bits(y))
    assert float(grads[0][1]) > 0.0


def test_mas_refusals():
    from mafed_amd import MAS, Trainer
    cfg, sd, _, batch, _ = golden_setup("t64")
    model = _model(cfg, sd)
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, MAS(), _conf(), reducer=types.SimpleNamespace(world=2))   # a stub: refused before anything looks at it
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, MAS(), _conf(), ddp=True)
    Trainer(model, MAS(), _conf())
    foreign = torch.nn.Linear(2, 2).to(DEV)
    mas = MAS()
    for call in (lambda: mas.update(foreign, dataloader=[]), lambda: mas.compute_importances(foreign, []),
                 lambda: mas.update_after_backward(model=foreign), lambda: mas.named(foreign)):
        with pytest.raises(TypeError, match="native model"):
            call()
    with pytest.raises(ValueError, match="dataloader"):
        mas.update(model)
    with pytest.raises(ValueError, match="alpha"):
        MAS(alpha=1.5)
    model.head_loss = "mse"   # (not a HeadLoss)
    with pytest.raises(ValueError, match="head_loss"):
        model(**_to_dev(batch), return_dict=True)
    model.head_loss = None
    assert float(model(**_to_dev(batch), return_dict=True).loss.detach()) > 0
