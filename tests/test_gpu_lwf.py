"""LwF (mafed_amd/methods/lwf.py) through the model and the Trainer: the step with a logit teacher against the oracle under torch
autograd, the row-sparse head against the dense head, the rows the teacher's head runs on, and the plugin's life inside Trainer.step."""
import types

import numpy as np
import pytest
import torch

from oracle import vlpythia_ref as R
from tests.helpers import assert_rel_close, golden_setup, tiny_cfg
from tests.kd_ref import kd_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3   # the project's fp32 gate


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


def _conf(lr=1e-3, accumulate=1):
    return types.SimpleNamespace(accumulate_grad_batches=accumulate, replay_interval=1, grad_norm=2.0, learning_rate=lr, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_steps=0, total_steps=100)


def _lwf_pair(cfg, teacher_sd, student_sd, dtype, lam, tau):
    """A model that finished a task with ``teacher_sd`` (LwF.update snapshots it) and then moved on to ``student_sd``."""
    from mafed_amd import CLMethod
    from mafed_amd.head_loss import LogitDistillation
    model = _model(cfg, teacher_sd, dtype)
    lwf = CLMethod["lwf"](reg_lambda=lam, temperature=tau)
    lwf.update(model)
    assert lwf.task_id == 1 and isinstance(model.head_loss, LogitDistillation) and lwf.past_model.head_loss is None
    assert not lwf.past_model.training and lwf.past_model is not model
    model.load_state_dict(student_sd, strict=True)
    return model, lwf


# t64: head size 64, left padding; t128: head size 128
@pytest.mark.parametrize("name", ["t64", "t128"])
def test_lwf_step_vs_oracle_autograd(name):
    """Teacher = the golden weights, student = teacher + seeded N(0, 1e-2).  Loss, its two parts, per-parameter gradient norms and three
    full gradients of one fp32 step against the oracle's float64 logits of both models with kd_ref's formula under torch autograd."""
    cfg, tsd, _, batch, _ = golden_setup(name)
    assert int((batch["attention_mask"][:, 0] == 0).sum()) > 0, "the case must have left padding"
    ssd = R.perturb(tsd, seed=777, std=1e-2)
    lam, tau = 0.7, 2.0
    params = {k: v.double().clone().requires_grad_(True) for k, v in ssd.items()}
    b64 = dict(batch, patch_embeddings=batch["patch_embeddings"].double())
    T = batch["input_ids"].shape[1]
    with torch.no_grad():
        t_logits = R.forward({k: v.double() for k, v in tsd.items()}, b64, cfg).logits[:, -T:]
    s_logits = R.forward(params, b64, cfg).logits[:, -T:]
    loss, ce, kd = kd_loss(s_logits, t_logits, batch["labels"], tau, lam)
    loss.backward()
    assert float(kd) > 0

    model, lwf = _lwf_pair(cfg, tsd, ssd, torch.float32, lam, tau)
    model.zero_grad()
    out = model(**_to_dev(batch), return_dict=True)
    got = lwf.compute_loss(model, out.loss, batch=batch)
    assert got is out.loss
    got.backward()
    torch.cuda.synchronize()
    assert_rel_close(out.loss, float(loss), TOL, f"{name} loss")
    assert_rel_close(lwf.last_ce, float(ce), TOL, f"{name} CE")
    assert_rel_close(lwf.last_kd, float(kd), TOL, f"{name} KD")
    assert_rel_close(model.last_head_losses, torch.stack([loss, ce, kd]).detach(), TOL, f"{name} last_head_losses")
    names = [k for k, _ in R.param_shapes(cfg)]
    norms = np.array([float(model._g(k).norm()) for k in names])
    assert_rel_close(norms, np.array([float(params[k].grad.norm()) for k in names]), TOL, f"{name} per-parameter gradient norms")
    last = cfg.num_hidden_layers - 1
    for k in ("embed_out.weight", f"gpt_neox.layers.{last}.mlp.dense_4h_to_h.weight", "gpt_neox.embed_in.weight"):
        assert_rel_close(model._g(k), params[k].grad, TOL, f"{name} grad {k}")


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
def test_sparse_head_equals_dense_head_with_a_logit_teacher(dtype, B, T, n_ans):
    """The same batch with and without ``max_label_rows``: equal loss and gradients (the bounds of the cross-entropy-only case in
    tests/test_gpu_sparse_head.py), and the teacher's head ran on the B * Rc compact rows, not on B * T."""
    from mafed_amd import CLMethod, VLPythiaConfig, VLPythiaForCausalLM
    cfg = VLPythiaConfig(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                         vision_hidden_size=32, num_vision_tokens=8)
    model = VLPythiaForCausalLM(cfg, compute_dtype=dtype, device=DEV, seed=5)
    lwf = CLMethod["lwf"](reg_lambda=1.0, temperature=2.0)
    lwf.update(model)
    gen = torch.Generator(device=DEV).manual_seed(6)
    with torch.no_grad():
        model.flat_params.add_(torch.randn(model.flat_params.shape, generator=gen, device=DEV) * 1e-2)
    model._shadow_dirty = True
    batch = _ragged_batch(cfg, B, T, n_ans, seed=B + T)
    seen = []
    inner = model.head_loss.teacher

    def spy(feats, ids, am, rows):
        out = inner(feats, ids, am, rows)
        seen.append((None if rows is None else rows.numel(), tuple(out[0].shape), out[0].dtype))
        return out

    model.head_loss.teacher = spy

    def run(hint):
        model.zero_grad()
        kw = {"max_label_rows": hint} if hint is not None else {}
        out = model(**batch, **kw, return_dict=True)
        out.loss.backward()
        torch.cuda.synchronize()
        return float(out.loss.detach()), model.flat_grads.clone(), model.last_head_losses.clone()

    l0, g0, h0 = run(None)
    l1, g1, h1 = run(n_ans)
    assert int(model.last_label_overflow) == 0 and float(h0[2]) > 0
    Rc = n_ans + 1 if dtype == torch.float32 else next(r for r in range(n_ans + 1, T + 1) if (B * r) % 128 == 0)
    V = cfg.vocab_size
    assert seen[0] == (None, (B, T, V), dtype), seen
    assert seen[1] == (B * Rc, (B * Rc, V), dtype) and B * Rc < B * T, seen
    tol = 1e-6 if dtype == torch.float32 else 2e-3
    assert abs(l1 - l0) <= tol * max(1.0, abs(l0)), (l0, l1)
    assert float((h1 - h0).abs().max()) <= tol * max(1.0, abs(l0)), (h0, h1)
    rel = float((g1 - g0).norm() / g0.norm())
    print(f"[lwf] sparse vs dense head, {dtype}: loss {l0} / {l1}, gradient relative difference {rel:.3e}")
    assert rel <= (1e-5 if dtype == torch.float32 else 1e-2), f"gradients: relative difference {rel:.3e}"


def _t64_batches(n, seed=300):
    cfg = tiny_cfg("t64")
    return cfg, [_to_dev(R.make_batch(cfg, 4, 6, seed=seed + i, pad=True, n_answer=3)) for i in range(n)]


def _checksum(model):
    return float(model.flat_params.double().abs().sum())


def test_lwf_before_the_first_update_is_naive():
    """No teacher during task 0: three Trainer steps give the loss bits and the parameter checksum of Naive."""
    from mafed_amd import CLMethod, Trainer
    cfg, batches = _t64_batches(3)
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    res = {}
    for key in ("naive", "lwf"):
        model = _model(cfg, sd)
        method = CLMethod[key]()
        tr = Trainer(model, method, _conf(), task_id=0)
        losses = [tr.step(dict(b), i)["loss"] for i, b in enumerate(batches)]
        tr.join()
        torch.cuda.synchronize()
        res[key] = ([float(x) for x in losses], _checksum(model))
        if key == "lwf":
            assert model.head_loss is None and float(method.last_kd) == 0.0 and float(method.last_ce) == res[key][0][-1]
    assert res["lwf"][0] == res["naive"][0], res
    assert res["lwf"][1] == res["naive"][1], res


def test_lwf_in_the_trainer_after_update():
    """First step after update(model): the student IS the teacher -- KD == 0.0 exactly, loss == CE; the optimiser step moves the
    student away and the next step has KD > 0."""
    from mafed_amd import CLMethod, Trainer
    cfg, batches = _t64_batches(2, seed=320)
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    model = _model(cfg, sd)
    lwf = CLMethod["lwf"](reg_lambda=1.0, temperature=2.0)
    lwf.update(model)
    tr = Trainer(model, lwf, _conf(), task_id=1)
    rec = tr.step(dict(batches[0]), 0)
    torch.cuda.synchronize()
    assert rec["branch"] == "task" and rec["stepped"]
    assert float(lwf.last_kd) == 0.0, float(lwf.last_kd)
    assert float(rec["loss"]) == float(lwf.last_ce)
    rec = tr.step(dict(batches[1]), 1)
    tr.join()
    torch.cuda.synchronize()
    kd, ce = float(lwf.last_kd), float(lwf.last_ce)
    assert kd > 0.0 and abs(float(rec["loss"]) - (ce + 1.0 * 2.0 ** 2 * kd)) <= 1e-5 * max(1.0, ce), (float(rec["loss"]), ce, kd)
    # a second task: the teacher is replaced by a snapshot without a teacher of its own
    old = lwf.past_model
    lwf.update(model)
    assert lwf.task_id == 2 and lwf.past_model is not old and lwf.past_model.head_loss is None


def _bf16_steps(overwrite, accumulate=2, n_micro=8):
    from mafed_amd import Trainer
    cfg, batches = _t64_batches(n_micro, seed=340)
    tsd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    student, lwf = _lwf_pair(cfg, tsd, R.perturb(tsd, seed=4, std=5e-3), torch.bfloat16, 1.0, 2.0)
    student.dw_group_layers = 2
    tr = Trainer(student, lwf, _conf(lr=1e-3, accumulate=accumulate), task_id=1, overwrite_weight_grads=overwrite)
    assert tr._overwrite_ok() == overwrite
    losses, gns, kds = [], [], []
    for i in range(n_micro):
        rec = tr.step(dict(batches[i]), i)
        losses.append(float(rec["loss"]))
        kds.append(float(lwf.last_kd))
        if rec["stepped"]:
            gns.append(float(rec["grad_norm"]))
    tr.join()
    torch.cuda.synchronize()
    return losses, gns, student.flat_params.clone(), student, kds


def test_lwf_overwrite_mode_equals_zero_then_accumulate():
    """accumulate = 2 in bf16: the first micro-batch of a window writes the weight-matrix gradients.  Losses, the clip's gradient norms
    and the parameters after four optimiser steps equal the run that zeroes and accumulates (the bounds of tests/test_gpu_overwrite.py)."""
    a = _bf16_steps(True)
    b = _bf16_steps(False)
    assert min(a[4]) > 0.0
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), f"micro-batch {i}: loss {x} vs {y}"
    assert len(a[1]) == 4
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), f"step {i}: grad norm {x} vs {y}"
    d = float((a[2] - b[2]).abs().max())
    assert d <= 2e-5, f"parameters differ by {d} after 4 optimiser steps"
    assert a[3]._dw_stale and not b[3]._dw_stale


def test_lwf_bf16_step_tracks_the_fp32_kernels():
    """One bf16 step against the exact-fp32 kernels on the same weights and batch: loss within 1e-2, gradient cosine >= 0.995 (the
    bf16-vs-fp32 bounds of tests/test_gpu_fullsize.py)."""
    cfg, tsd, _, batch, _ = golden_setup("m64")
    ssd = R.perturb(tsd, seed=778, std=1e-2)
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        model, lwf = _lwf_pair(cfg, tsd, ssd, dtype, 1.0, 2.0)
        model.zero_grad()
        out = model(**_to_dev(batch), return_dict=True)
        out.loss.backward()
        torch.cuda.synchronize()
        res[dtype] = (float(out.loss.detach()), model.flat_grads.double().clone(), float(model.last_head_losses[2]))
    (l32, g32, k32), (l16, g16, k16) = res[torch.float32], res[torch.bfloat16]
    cos = float((g16 * g32).sum() / (g16.norm() * g32.norm()))
    print(f"[lwf] bf16 vs fp32: loss {l16} / {l32}, KD {k16} / {k32}, gradient cosine {cos:.6f}")
    assert k32 > 0 and abs(l16 - l32) <= 1e-2 * abs(l32), (l16, l32)
    assert cos >= 0.995, f"gradient direction bf16 vs fp32: cos = {cos:.5f}"
