"""GEM (mafed_amd/methods/gem.py, csrc/gem.hip): the plugin's hook against the whole-step float64 oracle, and its life inside
Trainer.step -- per-task memories, the decisions along the float64 trajectory, the norm hand-over to the clip."""
import types

import numpy as np
import pytest
import torch

from tests import gem_ref as G
from tests.helpers import assert_rel_close, golden_setup, trainer_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3   # the project's fp32 gate


def _bits(t):
    return t.contiguous().view(torch.int32)


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


def _gem(model, mems, cls=None, accumulate=1, margin=0.5, eps=1e-3, n_tasks=None, B=4):
    """A GEM (or ``cls``) with one finished task per batch of ``mems``, each task's memory holding exactly that batch: memory_per_task =
    batch_size = its B, so every draw is a permutation of it.  The features are stored in fp32 (the buffer's default is bf16), as the
    oracle sees them."""
    from mafed_amd import GEM
    from mafed_amd.methods import HBMReplayBuffer
    B = mems[0]["input_ids"].shape[0] if mems else B
    K = n_tasks or max(len(mems), 1)
    opts = types.SimpleNamespace(tasks=[str(i) for i in range(K + 1)], seed=11, batch_size=B, accumulate_grad_batches=accumulate)
    gem = (cls or GEM)(opts, memory_size=B * K, model_type="vlpythia", margin=margin, eps=eps)
    if mems:
        gem.mem_dataloader = HBMReplayBuffer(B, torch.device(DEV), seed=opts.seed, feature_dtype=torch.float32)
    for t, mem in enumerate(mems):
        gem.update(dict(mem), model=model)
        assert gem.task_id == t + 1 and len(gem.task_memories) == t + 1 and len(gem.task_memories[t]) == B
        assert gem.task_memories[t].data["patch_embeddings"].dtype == torch.float32
    return gem


def _backward_and_hook(key):
    name, seeds, margin = key
    cfg, sd, _, batch, _ = golden_setup(name)
    model = _model(cfg, sd)
    gem = _gem(model, [G.memory_batch(name, s) for s in seeds], margin=margin)
    model.zero_grad()
    model(**_to_dev(batch), return_dict=True).loss.backward()
    before = model.flat_grads.clone()
    gem.update_after_backward(model=model)
    torch.cuda.synchronize()
    return model, gem, before


@pytest.mark.parametrize("key", list(G.ORACLE_CASES), ids=lambda k: f"{k[0]}-{k[1][0]}-{k[1][1]}-m{k[2]}")
def test_gem_hook_vs_oracle(key):
    """The hook on the golden weights and batch with one memory batch per task (K = 2): the Gram, the decision, the coefficients and
    every parameter gradient against the float64 g + sum_k v_k r_k of the oracle's three gradients.  One case is not violated (bit
    identity), one has one constraint in the support, one both; the fourth runs the default margin."""
    ref = G.oracle_case(*key)
    sol = ref["solve"]
    violated, support = G.ORACLE_CASES[key]
    model, gem, before = _backward_and_hook(key)
    assert float(gem.last_violated) == float(violated) and float(gem.last_support) == float(support)
    assert gem.last_gram.dtype == torch.float64 and gem.last_gram.is_cuda and gem.last_coef.is_cuda
    assert_rel_close(gem.last_gram, ref["gram"], TOL, f"{key} gram", scale=ref["sabs"])
    assert bool((gem.last_coef[2:] == 0).all())
    if not violated:
        assert bool((gem.last_coef == 0).all())
        assert torch.equal(_bits(before), _bits(model.flat_grads))
        return
    assert_rel_close(gem.last_coef[:2], sol["v"], TOL, f"{key} v")
    assert [float(x) > key[2] for x in gem.last_coef[:2]] == [bool(sol["mask"] >> k & 1) for k in range(2)]
    for k in ref["names"]:
        g, rs = ref["g"][k], [r[k] for r in ref["refs"]]
        want = g + sum(float(v) * r for v, r in zip(sol["v"], rs))
        assert_rel_close(model._g(k), want, TOL, f"{key} grad {k}", scale=g.abs() + sum(abs(float(v)) * r.abs() for v, r in zip(sol["v"], rs)))
    assert not torch.equal(before, model.flat_grads)


CASE2 = ("t64", (902, 907), 0.0)


def test_gem_norm_handover_is_folded_and_used_up(monkeypatch):
    """After the hook the clip folds the projection pass's partials: no pass over the buffer, the norm of the buffer as it is."""
    from mafed_amd import FlatAdamW, ops
    model, gem, _ = _backward_and_hook(CASE2)
    assert model.final_grad_sumsq is not None
    opt = FlatAdamW(model)
    monkeypatch.setattr(ops, "gradnorm_clip", lambda *a, **k: pytest.fail("the clip read the gradient buffer"))
    norm = float(opt.clip_grad_norm_(2.0))
    want = float(model.flat_grads.double().norm())
    assert model.final_grad_sumsq is None
    assert abs(norm - want) <= 1e-6 * want, (norm, want)
    assert abs(float(opt.clip_out[1]) - min(1.0, 2.0 / (want + 1e-6))) <= 1e-6


def test_stale_norm_handover_is_dropped():
    """A backward behind the hook makes the handed-over partials stale: the sweep drops them and the clip reads the buffer as it now is."""
    from mafed_amd import FlatAdamW, ops
    cfg, sd, _, batch, _ = golden_setup("t64")
    model, gem, _ = _backward_and_hook(CASE2)
    stale = float(ops.gradnorm_finish(model.final_grad_sumsq, 2.0, torch.empty(2, device=DEV))[0])
    model(**_to_dev(batch), return_dict=True).loss.backward()   # accumulates onto g~
    assert model.final_grad_sumsq is None
    opt = FlatAdamW(model)
    norm = float(opt.clip_grad_norm_(2.0))
    torch.cuda.synchronize()
    want = float(model.flat_grads.double().norm())
    assert norm == float(ops.gradnorm_clip(model.flat_grads, 2.0)[0])
    assert abs(norm - want) <= 1e-6 * want, (norm, want)
    assert abs(stale - want) > 1e-2 * want, "the case cannot tell the stale norm from the current one"


def test_gem_before_first_update_is_naive():
    """Task 0, no memory: three Trainer steps give the loss bits and the parameters of Naive (the run with the same one-pass norm form,
    as the plugin declares ``grads_only_through_model = False``), and nothing of the plugin's is allocated."""
    from mafed_amd import Naive, Trainer
    from oracle import vlpythia_ref as R
    from tests.helpers import tiny_cfg
    cfg = tiny_cfg("t64")
    batches = [_to_dev(R.make_batch(cfg, 4, 6, seed=300 + i, pad=True, n_answer=3)) for i in range(3)]
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    res = {}
    for key in ("naive", "gem"):
        model = _model(cfg, sd)
        method = _gem(model, [], n_tasks=2) if key == "gem" else Naive()
        tr = Trainer(model, method, _conf(), task_id=0, incremental_norm=False)
        losses = [tr.step(dict(b), i)["loss"] for i, b in enumerate(batches)]
        tr.join()
        torch.cuda.synchronize()
        res[key] = ([float(x) for x in losses], model.flat_params.clone())
        if key == "gem":
            assert method.last_coef is None and method._stash is None and model.final_grad_sumsq is None
    assert res["gem"][0] == res["naive"][0], res
    assert torch.equal(_bits(res["gem"][1]), _bits(res["naive"][1]))


def _torch_double(base):
    class TorchGEM(base):
        """The same stash / zero / memory backwards, then Gram, solve (tests/gem_ref.py, on the host) and projection in float64, rounded
        to fp32 once.  No hand-over: the clip takes the one-pass norm."""

        def update_after_backward(self, model=None, **kwargs):
            g = model.flat_grads.double()
            refs = []
            for mem in self.task_memories:
                model.zero_grad()
                model(**next(iter(mem)), compute_loss=True, return_dict=True).loss.backward()
                refs.append(model.flat_grads.double())
            X = torch.stack([g] + refs)
            sol = G.gem_solve((X @ X.t()).cpu().numpy(), self.margin, self.eps)
            if sol["violated"]:
                g = g + sum(float(v) * r for v, r in zip(sol["v"], refs))
            model.flat_grads.copy_(g.float())
            self.last_violated = torch.tensor(float(sol["violated"]))
            self.last_support = torch.tensor(float(sol["support"]))
            self.last_coef = torch.tensor(list(sol["v"]) + [0.0] * (8 - len(sol["v"])))
    return TorchGEM


def _trainer_run(cls):
    from mafed_amd import Trainer
    c = G.GEM_TRAINER
    cfg, sd, _, batches = trainer_case()
    model = _model(cfg, sd)
    gem = _gem(model, [batches[i][1] for i in c["memories"]], cls=cls, accumulate=c["accumulate"], margin=c["margin"], eps=c["eps"])
    tr = Trainer(model, gem, _conf(lr=c["lr"], accumulate=c["accumulate"]), task_id=2)
    losses, gns, decisions, coefs, one_pass = [], [], [], [], []
    for i in range(c["n_micro"]):
        rec = tr.step(_to_dev(batches[i][0]), i)
        assert rec["branch"] == "task"
        assert torch.is_tensor(rec["loss"]) and rec["loss"].is_cuda   # the step records stay device tensors
        losses.append(rec["loss"])
        if rec["stepped"]:
            assert rec["grad_norm"].is_cuda
            gns.append(rec["grad_norm"])
            decisions.append((gem.last_violated.clone(), gem.last_support.clone()))
            coefs.append(gem.last_coef.clone())
    tr.join()
    torch.cuda.synchronize()
    f = lambda xs: [float(x) for x in xs]
    return dict(loss=f(losses), gn=f(gns), decisions=[(bool(v), int(s)) for v, s in decisions], coefs=[c_.double().cpu().numpy() for c_ in coefs],
                params=model.flat_params.clone())


def test_gem_trainer_matches_fp64_oracle_and_torch_double():
    """Four optimiser steps at accumulate = 2, fp32, two finished tasks (tests/gem_ref.py::GEM_TRAINER), against (1) the float64 oracle's
    own trajectory -- the decision and the support of every step, the coefficients, the clip's grad norms -- and (2) a twin Trainer whose
    plugin does Gram, solve and projection in float64 on the same fp32 gradients, at the gates of tests/test_gpu_agem.py's Trainer
    test: losses 1e-6, grad norms 1e-5, parameters 1e-6 absolute."""
    from mafed_amd import GEM
    want = G.gem_trainer_fp64()
    a = _trainer_run(GEM)
    b = _trainer_run(_torch_double(GEM))
    pattern = [(v, bin(m).count("1")) for v, m in G.GEM_TRAINER_PATTERN]
    print(f"[gem] trainer: decisions {a['decisions']}, grad norms {a['gn']} / twin {b['gn']} / fp64 {[w['grad_norm'] for w in want]}")
    assert a["decisions"] == pattern and b["decisions"] == pattern
    assert len(a["loss"]) == 8 and len(a["gn"]) == 4
    for i, w in enumerate(want):
        v64, mask = w["solve"]["v"], w["solve"]["mask"]
        print(f"[gem] trainer step {i}: v {a['coefs'][i][:2]} / twin {b['coefs'][i][:2]} / fp64 {v64}")
        assert [x > G.GEM_TRAINER["margin"] for x in a["coefs"][i][:2]] == [bool(mask >> k & 1) for k in range(2)]
        assert not a["coefs"][i][2:].any()
        assert np.abs(a["coefs"][i][:2] - v64).max() <= TOL * max(np.abs(v64).max(), 1e-300) or not w["solve"]["violated"]
        assert np.abs(a["coefs"][i][:2] - b["coefs"][i][:2]).max() <= 1e-5 * max(np.abs(b["coefs"][i][:2]).max(), 1e-300) or not w["solve"]["violated"]
        assert abs(a["gn"][i] - w["grad_norm"]) <= 1e-5 * w["grad_norm"], f"step {i}: grad norm {a['gn'][i]} vs fp64 {w['grad_norm']}"
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert abs(x - y) <= 1e-6 * abs(y), f"micro-batch {i}: loss {x} vs {y}"
    for i, (x, y) in enumerate(zip(a["gn"], b["gn"])):
        assert abs(x - y) <= 1e-5 * abs(y), f"step {i}: grad norm {x} vs {y}"
    d = float((a["params"] - b["params"]).abs().max())
    print(f"[gem] trainer: parameters differ by {d:.3e} after 4 optimiser steps")
    assert d <= 1e-6, f"parameters differ by {d} after 4 optimiser steps"


def test_gem_grad_norm_is_the_norm_of_the_projected_gradient(monkeypatch):
    """rec["grad_norm"] of a violated step equals the one-pass norm of the buffer the hook left (and the clip made no pass of its own:
    the hand-over is really used), not the norm of the window's gradient."""
    from mafed_amd import GEM, Trainer, ops
    cfg, sd, _, batch, _ = golden_setup("t64")
    model = _model(cfg, sd)
    gem = _gem(model, [G.memory_batch("t64", s) for s in CASE2[1]], margin=CASE2[2])
    seen = {"passes": 0}
    hook, one_pass = GEM.update_after_backward, ops.gradnorm_clip

    def counted(*a, **k):
        seen["passes"] += 1
        return one_pass(*a, **k)

    def spy(self, model=None, **kw):
        seen["before"] = one_pass(model.flat_grads, 2.0).clone()
        hook(self, model=model, **kw)
        seen["after"] = one_pass(model.flat_grads, 2.0).clone()
    monkeypatch.setattr(GEM, "update_after_backward", spy)
    monkeypatch.setattr(ops, "gradnorm_clip", counted)
    tr = Trainer(model, gem, _conf(), task_id=2)
    rec = tr.step(_to_dev(batch), 0)
    tr.join()
    torch.cuda.synchronize()
    assert rec["stepped"] and float(gem.last_violated) == 1.0 and seen["passes"] == 0
    got, after, before = float(rec["grad_norm"]), float(seen["after"][0]), float(seen["before"][0])
    assert abs(got - after) <= 1e-6 * after, (got, after)
    assert abs(before - after) > 1e-3 * after, "the case cannot tell the projected gradient's norm from the window's"


def test_gem_refuses_a_reducer():
    from mafed_amd import Trainer
    cfg, sd, _, batch, _ = golden_setup("t64")
    model = _model(cfg, sd)
    gem = _gem(model, [batch])
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, gem, _conf(), task_id=1, reducer=types.SimpleNamespace(world=2))   # a stub: refused before anything looks at it
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, gem, _conf(), task_id=1, ddp=True)
    Trainer(model, gem, _conf(), task_id=1)


def test_gem_memories_stay_with_their_task_and_a_ninth_is_refused():
    """Eight tasks with disjoint token ids: every per-task buffer draws only its own task's samples, the stored samples are ER's under
    the same seed, the hook runs with K = 8, and a ninth ``update`` raises and changes nothing."""
    from mafed_amd import ER
    cfg, sd, _, batch, _ = golden_setup("t64")
    model = _model(cfg, sd)
    B, T = batch["input_ids"].shape
    span = (cfg.vocab_size - 1) // 9

    def task(t, n=2 * B):
        gen = torch.Generator().manual_seed(400 + t)
        pick = torch.randint(0, B, (n,), generator=gen)
        d = {k: v[pick].clone() for k, v in batch.items()}
        ids = torch.randint(1 + t * span, 1 + (t + 1) * span, (n, T), generator=gen)
        d["labels"] = torch.where(d["labels"] >= 0, ids, d["labels"])
        d["input_ids"] = torch.where(d["attention_mask"] > 0, ids, d["input_ids"])
        return d
    opts = types.SimpleNamespace(tasks=[str(i) for i in range(9)], seed=11, batch_size=B)
    er = ER(opts, memory_size=8 * B, model_type="vlpythia")
    gem = _gem(model, [], n_tasks=8, B=B)
    from mafed_amd.methods import HBMReplayBuffer
    for m in (er, gem):   # fp32 features, as the fp32 model of this test takes them
        m.mem_dataloader = HBMReplayBuffer(B, torch.device(DEV), seed=opts.seed, feature_dtype=torch.float32)
    for t in range(8):
        er.update(task(t), model=model)
        gem.update(task(t), model=model)
        assert torch.equal(gem.datasets[t]["input_ids"], er.datasets[t]["input_ids"])
    assert torch.equal(gem.mem_dataloader.data["input_ids"], er.mem_dataloader.data["input_ids"])
    for t, mem in enumerate(gem.task_memories):
        for _ in range(3):
            b = next(iter(mem))
            ids = b["input_ids"][b["attention_mask"] > 0]
            assert int(ids.min()) >= 1 + t * span and int(ids.max()) < 1 + (t + 1) * span
    model.zero_grad()
    model(**_to_dev(batch), return_dict=True).loss.backward()
    gem.update_after_backward(model=model)
    torch.cuda.synchronize()
    assert gem.last_gram.shape == (9, 9) and len(gem._refs) == 7 and bool(torch.isfinite(gem.last_gram).all())
    assert bool(torch.isfinite(model.flat_grads).all()) and float(gem.last_violated) in (0.0, 1.0)
    state = (gem.task_id, len(gem.datasets), len(gem.task_memories), len(gem.mem_dataloader))
    with pytest.raises(RuntimeError, match="GEM_MAX_REFS"):
        gem.update(task(8), model=model)
    assert state == (gem.task_id, len(gem.datasets), len(gem.task_memories), len(gem.mem_dataloader))
