"""DER++ (mafed_amd/methods/der.py) through the model and the Trainer: the recording pass and the replay step against the oracle under
torch autograd, the row-sparse head against the dense head, the plugin's life inside Trainer.step, a store that grows, and its state.

Nothing here runs on more than one process."""
import types

import numpy as np
import pytest
import torch

from oracle import vlpythia_ref as R
from tests.der_ref import der_loss, der_ref, rank_map
from tests.helpers import assert_rel_close, golden_setup, tiny_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3   # the project's fp32 gate
KEYS = ("input_ids", "attention_mask", "labels", "patch_embeddings")


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


def _conf(lr=1e-3, accumulate=1, replay_interval=1):
    return types.SimpleNamespace(accumulate_grad_batches=accumulate, replay_interval=replay_interval, grad_norm=2.0, learning_rate=lr,
                                 betas=(0.9, 0.98), weight_decay=0.01, optim="adamw", warmup_steps=0, total_steps=100)


def _der(batch_size, memory_size, n_tasks=2, accumulate=1, **kw):
    from mafed_amd import DER
    opts = types.SimpleNamespace(tasks=[str(i) for i in range(n_tasks)], seed=11, batch_size=batch_size, accumulate_grad_batches=accumulate)
    return DER(opts, memory_size=memory_size, model_type="vlpythia", **kw)


def _buffer_cpu(der, idx=None):
    """The buffer's own samples (all, or ``idx``) on the CPU, the features as the buffer keeps them (bf16) upcast to float64."""
    data = {k: der.mem_dataloader.data[k].cpu() for k in KEYS}
    if idx is not None:
        data = {k: v[idx] for k, v in data.items()}
    data["patch_embeddings"] = data["patch_embeddings"].double()
    return data


def _oracle_answer_logits(sd, cfg, data, A):
    """[N, A, V] float64: the oracle's logits of ``sd`` on the labelled rows of ``data``, in rank order; zeros in unused slots."""
    T = data["input_ids"].shape[1]
    with torch.no_grad():
        logits = R.forward({k: v.double() for k, v in sd.items()}, data, cfg).logits[:, -T:]
    want = torch.zeros(logits.shape[0], A, logits.shape[2], dtype=torch.float64)
    used = torch.zeros(logits.shape[0], A, dtype=torch.bool)
    for b, t, j in rank_map(data["labels"]):
        want[b, j], used[b, j] = logits[b, t], True
    return want, used


def _spy_ce_mse(monkeypatch):
    """Record (logits shape, mem_index, labels, out3) of every ops.ce_mse_fwd call."""
    from mafed_amd import ops
    seen, inner = [], ops.ce_mse_fwd

    def spy(logits, store, mem_index, labels, alpha, beta, poison=None):
        out = inner(logits, store, mem_index, labels, alpha, beta, poison=poison)
        seen.append({"shape": tuple(logits.shape), "logits": logits.detach().clone(), "mem_index": mem_index.clone(), "labels": labels.clone(),
                     "out3": out[0].clone()})
        return out

    monkeypatch.setattr(ops, "ce_mse_fwd", spy)
    return seen


# t64: head size 64, left padding; t128: head size 128
@pytest.mark.parametrize("name", ["t64", "t128"])
def test_recorded_logits_equal_the_oracle_on_the_labelled_rows(name):
    """After ``update`` the store holds the finished model's logits on every sample's labelled rows in rank order (the oracle's float64
    logits of the same weights), zeros in the unused slots; row n of the store is sample n of the buffer.  Recorded in two batches."""
    cfg, _, tsd, batch, _ = golden_setup(name)
    if name == "t64":
        assert int((batch["attention_mask"][:, 0] == 0).sum()) > 0, "the case must have left padding"
    labels = batch["labels"].clone()
    labels[-1, -2] = -100   # one sample with fewer labelled rows than the others, and a gap: an unused slot, rank != offset
    batch = dict(batch, labels=labels)
    N = batch["input_ids"].shape[0]
    model = _model(cfg, tsd)
    der = _der(batch_size=2, memory_size=N)
    der.update(batch, model=model)
    torch.cuda.synchronize()
    A = int((labels[:, 1:] != -100).sum(1).max())
    assert der.task_id == 1 and len(der.mem_dataloader) == N and der.mem_dataloader.attach_index
    assert der.logits.shape == (N, A, cfg.vocab_size) and der.logits.dtype == torch.float32 and der.logits.is_contiguous()
    data = _buffer_cpu(der)
    assert torch.equal(data["input_ids"], batch["input_ids"])   # (a dict dataset is taken in sorted order: buffer sample n is sample n)
    want, used = _oracle_answer_logits(tsd, cfg, data, A)
    assert not bool(used.all()) and bool(used[:, 0].all())
    assert_rel_close(der.logits, want, TOL, f"{name} recorded logits")
    assert float(der.logits[~used.to(DEV)].abs().max()) == 0.0, "unused slots must hold zeros"
    for n in range(N):   # per sample: a store in another order would pass a whole-tensor bound only by accident
        assert_rel_close(der.logits[n][used[n].to(DEV)], want[n][used[n]], TOL, f"{name} sample {n}")


@pytest.mark.parametrize("name", ["t64", "t128"])
def test_der_step_vs_oracle_autograd(name, monkeypatch):
    """The golden (teacher) weights record the store, the student is teacher + seeded N(0, 1e-2).  Loss, its two parts, per-parameter
    gradient norms and three full gradients of one fp32 replay step against ``der_loss`` on the oracle's float64 student logits and the
    plugin's own store under torch autograd."""
    cfg, _, tsd, batch, _ = golden_setup(name)
    ssd = R.perturb(tsd, seed=777, std=1e-2)
    alpha, beta = 0.5, 1.0
    N = batch["input_ids"].shape[0]
    model = _model(cfg, tsd)
    der = _der(batch_size=N, memory_size=N, alpha=alpha, beta=beta)
    der.update(batch, model=model)
    model.load_state_dict(ssd, strict=True)
    seen = _spy_ce_mse(monkeypatch)
    model.zero_grad()
    loss_got, n_ex = der.replay(model)
    loss_got.backward()
    torch.cuda.synchronize()
    assert n_ex == N and len(seen) == 1 and model.head_loss is None
    idx = seen[0]["mem_index"].cpu()
    assert sorted(idx.tolist()) == list(range(N))

    params = {k: v.double().clone().requires_grad_(True) for k, v in ssd.items()}
    b64 = _buffer_cpu(der, idx)
    T = b64["input_ids"].shape[1]
    s_logits = R.forward(params, b64, cfg).logits[:, -T:]
    loss, ce, mse = der_loss(s_logits, der.logits.cpu(), idx, b64["labels"], alpha, beta)
    loss.backward()
    assert float(mse.detach()) > 0
    assert_rel_close(loss_got, float(loss), TOL, f"{name} loss")
    assert_rel_close(der.last_ce, float(ce), TOL, f"{name} CE")
    assert_rel_close(der.last_mse, float(mse), TOL, f"{name} MSE")
    assert_rel_close(model.last_head_losses, torch.stack([loss, ce, mse]).detach(), TOL, f"{name} last_head_losses")
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
def test_sparse_head_equals_dense_head_with_a_logit_anchor(dtype, B, T, n_ans, monkeypatch):
    """The same memory batch with and without ``max_label_rows``: equal loss and gradients (the bounds of
    tests/test_gpu_lwf.py::test_sparse_head_equals_dense_head_with_a_logit_teacher); the sparse run's head ran on the B * Rc compact rows.
    The store is the model's own recording in a shuffled order, addressed through ``mem_index``."""
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    from mafed_amd.head_loss import LogitAnchor
    cfg = VLPythiaConfig(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                         vision_hidden_size=32, num_vision_tokens=8)
    model = VLPythiaForCausalLM(cfg, compute_dtype=dtype, device=DEV, seed=5)
    batch = _ragged_batch(cfg, B, T, n_ans, seed=B + T)
    z = model.answer_logits(batch["patch_embeddings"], batch["input_ids"], batch["attention_mask"], batch["labels"], n_ans)
    assert z.shape == (B, n_ans, cfg.vocab_size) and z.dtype == dtype
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(DEV)
    store = torch.empty_like(z)
    store[perm] = z   # sample b lives in row perm[b]
    gen = torch.Generator(device=DEV).manual_seed(6)
    with torch.no_grad():
        model.flat_params.add_(torch.randn(model.flat_params.shape, generator=gen, device=DEV) * 1e-2)
    model._shadow_dirty = True
    seen = _spy_ce_mse(monkeypatch)
    model.head_loss = LogitAnchor(store, perm, 0.5, 1.0)

    def run(hint):
        model.zero_grad()
        kw = {"max_label_rows": hint} if hint is not None else {}
        out = model(**batch, **kw, return_dict=True)
        out.loss.backward()
        torch.cuda.synchronize()
        return float(out.loss.detach()), model.flat_grads.clone(), model.last_head_losses.clone()

    l0, g0, h0 = run(None)
    l1, g1, h1 = run(n_ans)
    model.head_loss = None
    assert int(model.last_label_overflow) == 0 and float(h0[2]) > 0
    Rc = n_ans + 1 if dtype == torch.float32 else next(r for r in range(n_ans + 1, T + 1) if (B * r) % 128 == 0)
    V = cfg.vocab_size
    assert seen[0]["shape"] == (B, T, V) and seen[1]["shape"] == (B, Rc, V) and B * Rc < B * T, [s["shape"] for s in seen]
    tol = 1e-6 if dtype == torch.float32 else 2e-3
    assert abs(l1 - l0) <= tol * max(1.0, abs(l0)), (l0, l1)
    assert float((h1 - h0).abs().max()) <= tol * max(1.0, abs(l0)), (h0, h1)
    rel = float((g1 - g0).norm() / g0.norm())
    print(f"[der] sparse vs dense head, {dtype}: loss {l0} / {l1}, gradient relative difference {rel:.3e}")
    assert rel <= (1e-5 if dtype == torch.float32 else 1e-2), f"gradients: relative difference {rel:.3e}"
    # against the store in its recorded order the MSE is another number: the index is what pairs the rows
    model.head_loss = LogitAnchor(z, perm, 0.5, 1.0)
    try:
        with torch.enable_grad():
            model(**batch, return_dict=True)
    finally:
        model.head_loss = None
    assert abs(float(model.last_head_losses[2]) - float(h0[2])) > 1e-2 * float(h0[2])


def _t64_batches(n, seed=300):
    cfg = tiny_cfg("t64")
    return cfg, [_to_dev(R.make_batch(cfg, 4, 6, seed=seed + i, pad=True, n_answer=3)) for i in range(n)]


def _checksum(model):
    return float(model.flat_params.double().abs().sum())


def test_der_before_the_first_update_is_naive():
    """No memory during task 0: three Trainer steps give the loss bits and the parameter checksum of Naive."""
    from mafed_amd import CLMethod, Trainer
    cfg, batches = _t64_batches(3)
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    res = {}
    for key in ("naive", "der"):
        model = _model(cfg, sd)
        method = CLMethod[key]() if key == "naive" else _der(batch_size=4, memory_size=4)
        tr = Trainer(model, method, _conf(), task_id=0)
        recs = [tr.step(dict(b), i) for i, b in enumerate(batches)]
        tr.join()
        torch.cuda.synchronize()
        assert all(r["branch"] == "task" for r in recs)
        res[key] = ([float(r["loss"]) for r in recs], _checksum(model))
        if key == "der":
            assert model.head_loss is None and method.logits is None and method.last_mse is None
    assert res["der"][0] == res["naive"][0], res
    assert res["der"][1] == res["naive"][1], res


def test_der_in_the_trainer_after_update(monkeypatch):
    """replay_interval = 1 in task 1: every step is a replay step -- the ce_mse kernels run, ce_fwd does not, loss == beta CE + alpha MSE,
    and ``head_loss`` is emptied afterwards, also when the forward raises.  With replay_interval = 2 the step in between is a task
    step: plain cross-entropy, the ce_mse kernels do not run."""
    from mafed_amd import Trainer, ops
    cfg, batches = _t64_batches(3, seed=320)
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    model = _model(cfg, sd)
    alpha, beta = 0.3, 0.7
    der = _der(batch_size=4, memory_size=4, alpha=alpha, beta=beta)
    der.update({k: v.cpu() for k, v in batches[2].items()}, model=model)
    model.load_state_dict(R.perturb(sd, seed=6, std=1e-2), strict=True)   # the student has moved on: MSE > 0
    tr = Trainer(model, der, _conf(replay_interval=1), task_id=1)
    real = {n: getattr(ops, n) for n in ("ce_fwd", "ce_mse_fwd", "ce_mse_bwd")}
    monkeypatch.setattr(ops, "ce_fwd", lambda *a, **k: pytest.fail("ce_fwd ran on a replay step"))
    rec = tr.step(dict(batches[0]), 0)
    tr.join()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "ce_fwd", real["ce_fwd"])
    assert rec["branch"] == "replay" and rec["stepped"] and model.head_loss is None
    ce, mse = float(der.last_ce), float(der.last_mse)
    assert mse > 0.0
    assert abs(float(rec["loss"]) - (beta * ce + alpha * mse)) <= 1e-5 * max(1.0, ce), (float(rec["loss"]), ce, mse)
    # a task step of the same trainer
    tr.replay_interval = 2
    for n in ("ce_mse_fwd", "ce_mse_bwd"):
        monkeypatch.setattr(ops, n, lambda *a, _n=n, **k: pytest.fail(f"{_n} ran on a task step"))
    rec = tr.step(dict(batches[1]), 0)
    tr.join()
    torch.cuda.synchronize()
    for n in ("ce_mse_fwd", "ce_mse_bwd"):
        monkeypatch.setattr(ops, n, real[n])
    assert rec["branch"] == "task" and rec["stepped"] and model.head_loss is None
    # a forward that raises (a store of another dtype) leaves no anchor behind
    der.logits = der.logits.to(torch.bfloat16)
    with pytest.raises(ValueError):
        der.replay(model)
    assert model.head_loss is None


def _bf16_steps(overwrite, accumulate=2, n_micro=8):
    from mafed_amd import Trainer
    cfg, batches = _t64_batches(n_micro, seed=340)
    tsd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    student = _model(cfg, tsd, torch.bfloat16)
    der = _der(batch_size=4, memory_size=8, accumulate=accumulate)
    mem = R.make_batch(cfg, 8, 6, seed=999, pad=True, n_answer=3)
    der.update(mem, model=student)
    student.load_state_dict(R.perturb(tsd, seed=4, std=5e-3), strict=True)
    student.dw_group_layers = 2
    tr = Trainer(student, der, _conf(lr=1e-3, accumulate=accumulate), task_id=1, overwrite_weight_grads=overwrite)
    assert tr._overwrite_ok() == overwrite
    losses, gns, mses = [], [], []
    for i in range(n_micro):
        rec = tr.step(dict(batches[i]), i)
        assert rec["branch"] == "replay"
        losses.append(float(rec["loss"]))
        mses.append(float(der.last_mse))
        if rec["stepped"]:
            gns.append(float(rec["grad_norm"]))
    tr.join()
    torch.cuda.synchronize()
    return losses, gns, student.flat_params.clone(), student, mses


def test_der_overwrite_mode_equals_zero_then_accumulate():
    """accumulate = 2 in bf16, every step a replay step: the first micro-batch of a window writes the weight-matrix gradients.  Losses, the
    clip's gradient norms and the parameters after four optimiser steps equal the run that zeroes and accumulates (the bounds of
    tests/test_gpu_lwf.py::test_lwf_overwrite_mode_equals_zero_then_accumulate)."""
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


def test_der_bf16_step_tracks_the_fp32_kernels():
    """One bf16 replay step against the exact-fp32 kernels on the same weights and memory: loss within 1e-2, gradient cosine >= 0.995
    (the bf16-vs-fp32 bounds of tests/test_gpu_fullsize.py)."""
    cfg, _, tsd, batch, _ = golden_setup("m64")   # (the case of tests/test_gpu_lwf.py::test_lwf_bf16_step_tracks_the_fp32_kernels)
    ssd = R.perturb(tsd, seed=778, std=1e-2)
    N = batch["input_ids"].shape[0]
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        model = _model(cfg, tsd, dtype)
        der = _der(batch_size=N, memory_size=N)
        der.update(batch, model=model)
        assert der.logits.dtype == dtype
        model.load_state_dict(ssd, strict=True)
        model.zero_grad()
        loss, _ = der.replay(model)
        loss.backward()
        torch.cuda.synchronize()
        res[dtype] = (float(loss.detach()), model.flat_grads.double().clone(), float(der.last_mse))
    (l32, g32, m32), (l16, g16, m16) = res[torch.float32], res[torch.bfloat16]
    cos = float((g16 * g32).sum() / (g16.norm() * g32.norm()))
    print(f"[der] bf16 vs fp32: loss {l16} / {l32}, MSE {m16} / {m32}, gradient cosine {cos:.6f}")
    assert m32 > 0 and abs(l16 - l32) <= 1e-2 * abs(l32), (l16, l32)
    assert cos >= 0.995, f"gradient direction bf16 vs fp32: cos = {cos:.5f}"


def test_a_second_update_grows_the_store(monkeypatch):
    """Task 1's samples have two labelled rows, task 2's have four and a longer text: A grows from 2 to 4, the earlier samples' stored
    rows stay bit for bit with zeros in the new slots, the new rows are the model's recording of the new buffer samples, and a
    replay step over the mixed memory matches ``der_ref`` on the model's own logits of the drawn batch."""
    cfg = tiny_cfg("t64")
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    model = _model(cfg, sd)
    der = _der(batch_size=8, memory_size=8, n_tasks=3, alpha=0.5, beta=1.0)
    der.update(R.make_batch(cfg, 4, 6, seed=501, pad=True, n_answer=2), model=model)
    first = der.logits.clone()
    assert first.shape == (4, 2, cfg.vocab_size)
    der.update(R.make_batch(cfg, 4, 8, seed=502, pad=True, n_answer=4), model=model)
    torch.cuda.synchronize()
    assert der.task_id == 2 and der.logits.shape == (8, 4, cfg.vocab_size) == (len(der.mem_dataloader), 4, cfg.vocab_size)
    assert torch.equal(der.logits[:4, :2], first) and float(der.logits[:4, 2:].abs().max()) == 0.0
    data = {k: v for k, v in der.mem_dataloader.data.items()}
    assert data["input_ids"].shape == (8, 8)   # (the earlier samples were left-padded to the longer text)
    again = model.answer_logits(data["patch_embeddings"], data["input_ids"], data["attention_mask"], data["labels"], 4)
    # (the first four were recorded at T = 6; two more masked positions between image and text move the text's rotary distance to the
    #  image, so their logits at T = 8 are other numbers -- the store keeps what the model gave when the sample was stored)
    for n in range(4, 8):
        assert_rel_close(der.logits[n], again[n], TOL, f"store row {n}")
    # a replay step with a student that has moved on
    model.load_state_dict(R.perturb(sd, seed=5, std=1e-2), strict=True)
    seen = _spy_ce_mse(monkeypatch)
    model.zero_grad()
    loss, n_ex = der.replay(model)
    loss.backward()
    torch.cuda.synchronize()
    idx = seen[0]["mem_index"]
    assert n_ex == 8 and sorted(idx.tolist()) == list(range(8))
    drawn = {k: v.index_select(0, idx) for k, v in data.items()}
    with torch.no_grad():
        logits = model(**drawn, return_dict=True).logits
    ref = der_ref(logits, der.logits, idx.cpu(), drawn["labels"], 0.5, 1.0)
    assert float(ref["out3"][2]) > 0
    assert_rel_close(model.last_head_losses, ref["out3"], TOL, "loss, CE, MSE over the mixed memory")
    assert_rel_close(model.last_head_losses[2], float(ref["out3"][2]), TOL, "MSE over the mixed memory")
    assert_rel_close(loss, float(ref["out3"][0]), TOL, "replay loss")


def test_state_round_trip():
    cfg, _, tsd, batch, _ = golden_setup("t64")
    N = batch["input_ids"].shape[0]
    model = _model(cfg, tsd)
    der = _der(batch_size=N, memory_size=N)
    assert der.state_dict() == {"logits": None, "task_id": 0}
    der.update(batch, model=model)
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in der.state_dict().items()}
    assert set(sd) == {"logits", "task_id"}
    other = _der(batch_size=N, memory_size=N)
    other.update(batch, model=model)
    other.logits.zero_()
    other.load_state_dict(sd)
    assert other.task_id == 1 and other.logits.device.type == "cuda" and torch.equal(other.logits, der.logits)
    assert other.logits.data_ptr() != der.logits.data_ptr()
    with pytest.raises(ValueError):
        other.load_state_dict({"logits": sd["logits"]})


def test_conflicting_and_mismatched_hooks_raise(monkeypatch):
    from mafed_amd import MAS, ops
    from mafed_amd.head_loss import LogitAnchor, LogitDistillation
    from mafed_amd.profiler import KernelProfile
    cfg, _, tsd, batch, _ = golden_setup("t64")
    model = _model(cfg, tsd)
    B, V = batch["input_ids"].shape[0], cfg.vocab_size
    store = torch.zeros(B, 4, V, device=DEV)
    idx = torch.arange(B, device=DEV)
    dev = _to_dev(batch)

    def forward():
        try:
            return model(**dev, return_dict=True)
        finally:
            torch.cuda.synchronize()

    model.head_loss = LogitAnchor(store, idx, 0.5, 1.0)
    assert forward().loss is not None
    model.head_loss = None
    # one head loss per step: a replay on a model whose slot is taken is refused before anything is launched, and the slot stays as it was
    der = _der(batch_size=B, memory_size=B)
    der.update(batch, model=model)
    torch.cuda.synchronize()
    taken = model.head_loss = LogitDistillation(lambda *a, **k: pytest.fail("the logit teacher ran beside a logit anchor"))
    real = {n: getattr(ops, n) for n in ("ce_mse_fwd", "ce_kd_fwd")}
    for n in real:
        monkeypatch.setattr(ops, n, lambda *a, _n=n, **k: pytest.fail(f"{_n} ran in a refused replay"))
    with KernelProfile() as prof:
        with pytest.raises(ValueError, match="LogitDistillation.*LogitAnchor.*one head loss per step"):
            der.replay(model)
    assert prof.records() == [] and model.head_loss is taken
    for n in real:
        monkeypatch.setattr(ops, n, real[n])
    for bad in ((store.to(torch.bfloat16), idx), (store[..., : V // 2].contiguous(), idx), (store, idx.to(torch.int32)), (store, idx[:-1])):
        model.head_loss = LogitAnchor(*bad, 0.5, 1.0)
        with pytest.raises(ValueError):
            forward()
    # an inference forward and the MAS importance pass do not look at the anchor
    malformed = model.head_loss = LogitAnchor(store.to(torch.bfloat16), idx, 0.5, 1.0)
    with torch.no_grad():
        assert forward().loss is not None
    for n in ("ce_mse_fwd", "ce_mse_bwd"):
        monkeypatch.setattr(ops, n, lambda *a, _n=n, **k: pytest.fail(f"{_n} ran in the MAS importance pass"))
    mas = MAS()
    mas.update(model, dataloader=[dev])
    torch.cuda.synchronize()
    assert mas.task_id == 1 and model.head_loss is malformed
    model.head_loss = None
