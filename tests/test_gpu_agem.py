"""A-GEM (mafed_amd/methods/agem.py, csrc/agem.hip): the two flat-buffer kernels against float64 numpy, the plugin's hook against the
whole-step oracle, and its life inside Trainer.step -- the norm hand-over to the clip included."""
import types

import numpy as np
import pytest
import torch

from tests.agem_ref import AGEM_TRAINER, ORACLE_CASES, agem_stats, memory_batch, oracle_case
from tests.helpers import assert_rel_close, golden_setup, trainer_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3   # the project's fp32 gate
EPS22 = 2.0 ** -22

# 0: empty; 1, 3: tail only; 4: one vector; 1023: less than one block; 4 * 1024 + 1: several blocks and a tail behind full vectors;
# 3 * 2^21 + 5: above 2 * 2048 * 256 * 4, so the grid-stride loop at the grid cap goes through its two-accumulator body and on
SIZES = [0, 1, 3, 4, 1023, 4 * 1024 + 1, 3 * 2 ** 21 + 5]
MODES = ["random", "violated", "same", "zero"]

_INPUTS = {}


def _inputs(n, mode):
    """(g, r) fp32 on the device and their float64 numpy copies; built once per case and left unchanged."""
    key = (n, mode)
    if key not in _INPUTS:
        gen = torch.Generator().manual_seed(1000 + n % 997 + 7 * MODES.index(mode))
        g = torch.randn(n, generator=gen)
        if n > 2:
            g[2] = -0.0
        if mode == "random":
            r = torch.randn(n, generator=gen)
        elif mode == "violated":
            r = -g + 0.5 * g.abs() * (2 * torch.rand(n, generator=gen) - 1)   # noise below |g| element by element: violated at every n
        elif mode == "same":
            r = g.clone()
        else:
            r = torch.zeros(n)
        _INPUTS[key] = (g.to(DEV), r.to(DEV), g.double().numpy(), r.double().numpy())
    return _INPUTS[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(g, r, alias):
    """dots + project on copies of the inputs -> (stats4, out, partials); ``alias``: out is r's buffer."""
    from mafed_amd import ops
    rr = r.clone()
    stats = ops.agem_dots(g, rr)
    partials = torch.full((ops.agem_blocks(g.numel()) + 3,), -7.0, device=DEV)
    out = ops.agem_project(g, rr, stats, out=rr if alias else None, sumsq_partials=partials)
    assert g.numel() == 0 or (out.data_ptr() == rr.data_ptr()) == alias
    return stats, out, partials


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_agem_kernels_vs_fp64(n, mode):
    from mafed_amd import ops
    g, r, g64, r64 = _inputs(n, mode)
    dot64, rsq64, _, viol64, sabs = agem_stats(g64, r64)
    stats, out, partials = _run(g, r, alias=False)
    stats_a, out_a, partials_a = _run(g, r, alias=True)
    stats_b, out_b, _ = _run(g, r, alias=False)
    torch.cuda.synchronize()
    # run to run, and into r's own buffer: the same bits
    assert torch.equal(_bits(stats), _bits(stats_b)) and torch.equal(_bits(out), _bits(out_b))
    assert torch.equal(_bits(stats), _bits(stats_a)) and torch.equal(_bits(out), _bits(out_a)) and torch.equal(_bits(partials), _bits(partials_a))
    dot, rsq, alpha, viol = (float(x) for x in stats.double().cpu())
    print(f"[agem] n {n} {mode}: dot {dot:.8g} (fp64 {dot64:.8g}, sum|g r| {sabs:.6g}), rsq {rsq:.8g} (fp64 {rsq64:.8g}), alpha {alpha:.8g}, violated {viol}")
    assert abs(dot - dot64) <= 1e-5 * sabs and abs(rsq - rsq64) <= 1e-5 * rsq64
    assert viol == (1.0 if (dot < 0 and rsq > 0) else 0.0)
    if abs(dot64) > 1e-5 * sabs:
        assert viol == float(viol64)
    if mode == "violated" and n:
        assert viol == 1.0
    if mode in ("same", "zero") or n == 0:
        assert viol == 0.0
    if viol:
        assert abs(alpha - dot / rsq) <= EPS22 * abs(dot / rsq)
        want = g64 - alpha * r64
        err = np.abs(out.double().cpu().numpy() - want)
        bound = EPS22 * (np.abs(g64) + np.abs(alpha * r64))
        assert bool((err <= bound).all()), f"out: worst excess {float((err - bound).max()):.3e}"
    else:
        assert alpha == 0.0
        assert torch.equal(out, g) and torch.equal(_bits(out), _bits(g))   # bit for bit: the -0.0 in g[2] stays -0.0
    # norm hand-over: the partials folded by gradnorm_finish against the one-pass norm of out
    nb = ops.agem_blocks(n)
    assert 1 <= nb <= 2048 and bool((partials[nb:] == -7.0).all())
    folded = ops.gradnorm_finish(partials[:nb], 2.0, torch.empty(2, device=DEV))
    ref64 = float(np.sqrt((out.double().cpu().numpy() ** 2).sum()))
    if n:
        one_pass = ops.gradnorm_clip(out, 2.0)
        for i, what in enumerate(("norm", "clip scale")):
            a, b = float(folded[i]), float(one_pass[i])
            assert abs(a - b) <= 1e-6 * abs(b), f"{what}: folded {a} vs one pass {b}"
        assert abs(float(folded[0]) - ref64) <= 1e-6 * ref64
    else:
        assert float(folded[0]) == 0.0 and float(folded[1]) == 1.0
        assert [dot, rsq, alpha, viol] == [0.0] * 4


def test_agem_kernels_do_not_hide_a_non_finite_reference():
    """One inf in r (arithmetic on data): alpha is NaN, out holds non-finite values and the folded norm marks the step as skipped."""
    from mafed_amd import ops
    g, r, _, _ = _inputs(4 * 1024 + 1, "random")
    r = r.clone()
    r[1234] = float("inf")
    stats, out, partials = _run(g, r, alias=True)
    folded = ops.gradnorm_finish(partials[:ops.agem_blocks(g.numel())], 2.0, torch.empty(2, device=DEV))
    torch.cuda.synchronize()
    assert not np.isfinite(float(stats[1])) and np.isnan(float(stats[2])) and float(stats[3]) == 1.0
    assert not bool(torch.isfinite(out).all())
    assert not np.isfinite(float(folded[0])) and float(folded[1]) == -1.0


def test_agem_kernels_refuse_misaligned_buffers():
    from mafed_amd import _lib, ops
    g, r, _, _ = _inputs(1023, "random")
    with pytest.raises(_lib.MafedHipError):
        ops.agem_dots(g[1:], r[1:])
    stats = ops.agem_dots(g, r)
    with pytest.raises(_lib.MafedHipError):
        ops.agem_project(g[1:], r[1:], stats)


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


def _conf(lr=1e-3, accumulate=1):
    return types.SimpleNamespace(accumulate_grad_batches=accumulate, replay_interval=1, grad_norm=2.0, learning_rate=lr, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_steps=0, total_steps=100)


def _agem(model, mem, cls=None, accumulate=1, fill=True):
    """An AGEM (or ``cls``) whose memory holds exactly the samples of ``mem``: memory_size = batch_size = its B, so every draw is a
    permutation of it.  The features are stored in fp32 (the buffer's default is bf16), as the oracle sees them."""
    from mafed_amd import AGEM
    from mafed_amd.methods import HBMReplayBuffer
    B = mem["input_ids"].shape[0]
    opts = types.SimpleNamespace(tasks=["a", "b"], seed=11, batch_size=B, accumulate_grad_batches=accumulate)
    agem = (cls or AGEM)(opts, memory_size=B, model_type="vlpythia")
    if fill:
        agem.mem_dataloader = HBMReplayBuffer(B, torch.device(DEV), seed=opts.seed, feature_dtype=torch.float32)
        agem.update(dict(mem), model=model)
        assert agem.task_id == 1 and len(agem.mem_dataloader) == B
    return agem


def _backward_and_hook(name, seed):
    cfg, sd, _, batch, _ = golden_setup(name)
    model = _model(cfg, sd)
    agem = _agem(model, memory_batch(name, seed))
    model.zero_grad()
    model(**_to_dev(batch), return_dict=True).loss.backward()
    before = model.flat_grads.clone()
    agem.update_after_backward(model=model)
    torch.cuda.synchronize()
    return model, agem, before


@pytest.mark.parametrize("name,seed", [k for k, s in ORACLE_CASES.items() if s < 0])
def test_agem_projection_vs_oracle(name, seed):
    """The hook on the golden weights and batch with the memory batch of the case: every parameter gradient against the float64
    g - (dot / rsq) r of the oracle's two gradients."""
    ref = oracle_case(name, seed)
    dot, rsq, alpha, violated, _ = ref["stats"]
    assert violated
    model, agem, before = _backward_and_hook(name, seed)
    assert float(agem.last_projected) == 1.0
    assert_rel_close(agem.last_alpha, alpha, TOL, f"{name}/{seed} alpha")
    assert_rel_close(agem.last_dot, dot, TOL, f"{name}/{seed} dot")
    assert_rel_close(agem.last_ref_sq, rsq, TOL, f"{name}/{seed} rsq")
    for k in ref["names"]:
        g, r = ref["g"][k], ref["r"][k]
        assert_rel_close(model._g(k), g - alpha * r, TOL, f"{name}/{seed} grad {k}", scale=g.abs() + abs(alpha) * r.abs())
    assert not torch.equal(before, model.flat_grads)


def test_agem_norm_handover_is_folded_and_used_up(monkeypatch):
    """After the hook the clip folds the projection pass's partials: no pass over the buffer, the norm of the buffer as it is."""
    from mafed_amd import FlatAdamW, ops
    model, agem, _ = _backward_and_hook("t64", 902)
    assert model.final_grad_sumsq is not None
    opt = FlatAdamW(model)
    monkeypatch.setattr(ops, "gradnorm_clip", lambda *a, **k: pytest.fail("the clip read the gradient buffer"))
    norm = float(opt.clip_grad_norm_(2.0))
    want = float(model.flat_grads.double().norm())
    assert model.final_grad_sumsq is None
    assert abs(norm - want) <= 1e-6 * want, (norm, want)
    assert abs(float(opt.clip_out[1]) - min(1.0, 2.0 / (want + 1e-6))) <= 1e-6


@pytest.mark.parametrize("name,seed", [k for k, s in ORACLE_CASES.items() if s > 0])
def test_agem_no_violation_is_identity(name, seed):
    assert not oracle_case(name, seed)["stats"][3]
    model, agem, before = _backward_and_hook(name, seed)
    assert float(agem.last_projected) == 0.0 and float(agem.last_alpha) == 0.0 and float(agem.last_dot) > 0.0
    assert torch.equal(_bits(before), _bits(model.flat_grads))


def test_stale_norm_handover_is_dropped():
    """A backward behind the hook makes the handed-over partials stale: the sweep drops them and the clip reads the buffer as it now is."""
    from mafed_amd import FlatAdamW, ops
    cfg, sd, _, batch, _ = golden_setup("t64")
    model, agem, _ = _backward_and_hook("t64", 902)
    stale = float(ops.gradnorm_finish(model.final_grad_sumsq, 2.0, torch.empty(2, device=DEV))[0])
    model(**_to_dev(batch), return_dict=True).loss.backward()   # accumulates onto g'
    assert model.final_grad_sumsq is None
    opt = FlatAdamW(model)
    norm = float(opt.clip_grad_norm_(2.0))
    torch.cuda.synchronize()
    want = float(model.flat_grads.double().norm())
    assert norm == float(ops.gradnorm_clip(model.flat_grads, 2.0)[0])
    assert abs(norm - want) <= 1e-6 * want, (norm, want)
    assert abs(stale - want) > 1e-2 * want, "the case cannot tell the stale norm from the current one"


def _checksum(model):
    return float(model.flat_params.double().abs().sum())


def test_agem_before_first_update_is_naive():
    """Task 0, empty memory: three Trainer steps give the loss bits and the parameter checksum of Naive.  The plugin declares
    ``grads_only_through_model = False``, so its Trainer takes the one-pass clip norm: the Naive run it equals bit for bit is the one with
    the same norm form (incremental_norm=False); against the default Naive run, whose norm is summed in another order, it agrees to
    rounding."""
    from mafed_amd import Naive, Trainer
    from oracle import vlpythia_ref as R
    from tests.helpers import tiny_cfg
    cfg = tiny_cfg("t64")
    batches = [_to_dev(R.make_batch(cfg, 4, 6, seed=300 + i, pad=True, n_answer=3)) for i in range(3)]
    sd = R.init_weights(cfg, seed=3, bias_std=0.02, ln_jitter=0.05)
    res = {}
    for key in ("naive", "naive_default_norm", "agem"):
        model = _model(cfg, sd)
        method = _agem(model, batches[0], fill=False) if key == "agem" else Naive()
        tr = Trainer(model, method, _conf(), task_id=0, incremental_norm=key != "naive")
        losses = [tr.step(dict(b), i)["loss"] for i, b in enumerate(batches)]
        tr.join()
        torch.cuda.synchronize()
        res[key] = ([float(x) for x in losses], _checksum(model), model.flat_params.clone())
        if key == "agem":
            assert method.last_alpha is None and method._stash is None and model.final_grad_sumsq is None
    assert res["agem"][0] == res["naive"][0], res
    assert res["agem"][1] == res["naive"][1], res
    for a, b in zip(res["agem"][0], res["naive_default_norm"][0]):
        assert abs(a - b) <= 1e-5 * abs(b)
    assert float((res["agem"][2] - res["naive_default_norm"][2]).abs().max()) <= 1e-6


def _torch_double(base):
    class TorchAGEM(base):
        """The same stash / zero / memory backward, then the projection with torch ops in float64, rounded to fp32.  No hand-over: the
        clip takes the one-pass norm."""

        def update_after_backward(self, model=None, **kwargs):
            g = model.flat_grads.clone()
            model.zero_grad()
            batch = next(iter(self.mem_dataloader))
            model(**batch, compute_loss=True, return_dict=True).loss.backward()
            r = model.flat_grads
            g64, r64 = g.double(), r.double()
            dot, rsq = (g64 * r64).sum(), (r64 * r64).sum()
            violated = bool(dot < 0) and bool(rsq > 0)
            r.copy_((g64 - (dot / rsq) * r64).float() if violated else g)
            self.last_projected = torch.tensor(1.0 if violated else 0.0)
            self.last_dot = dot
    return TorchAGEM


def _trainer_run(cls, dtype=torch.float32, overwrite=True):
    from mafed_amd import Trainer
    c = AGEM_TRAINER
    cfg, sd, _, batches = trainer_case()
    model = _model(cfg, sd, dtype)
    if dtype == torch.bfloat16:
        model.dw_group_layers = 2
    agem = _agem(model, batches[c["memory"]][1], cls=cls, accumulate=c["accumulate"])
    tr = Trainer(model, agem, _conf(lr=c["lr"], accumulate=c["accumulate"]), task_id=1, overwrite_weight_grads=overwrite)
    assert tr._overwrite_ok() == (overwrite and dtype == torch.bfloat16)
    losses, gns, projected, dots = [], [], [], []
    for i in range(c["n_micro"]):
        rec = tr.step(_to_dev(batches[i][0]), i)
        assert rec["branch"] == "task"
        assert torch.is_tensor(rec["loss"]) and rec["loss"].is_cuda   # the step records stay device tensors
        losses.append(rec["loss"])
        if rec["stepped"]:
            assert rec["grad_norm"].is_cuda
            gns.append(rec["grad_norm"])
            projected.append(agem.last_projected.clone())
            dots.append(agem.last_dot.clone())
    tr.join()
    torch.cuda.synchronize()
    f = lambda xs: [float(x) for x in xs]
    return dict(loss=f(losses), gn=f(gns), projected=f(projected), dots=f(dots), params=model.flat_params.clone(), model=model)


def test_agem_trainer_matches_torch_double():
    """Four optimiser steps at accumulate = 2, fp32, task 1, against a twin Trainer whose plugin projects with torch ops in float64.
    Micro-batches 0 .. 7 of tests.helpers.trainer_case() (task-batch seeds 33 .. 40), the memory = its memory batch 1 (seed 74), both
    plugins' draws from the same seed.  The float64 oracle's dots along its own trajectory (tests/agem_ref.py::agem_trainer_fp64, checked
    on the CPU by tests/test_agem_ref.py): +2.651, -1.637, -0.874, +1.208, i.e. dot / sum|g r| = +0.133, -0.196, -0.197, +0.260 -- steps
    1 and 2 project, steps 0 and 3 do not."""
    from mafed_amd import AGEM
    a = _trainer_run(AGEM)
    b = _trainer_run(_torch_double(AGEM))
    print(f"[agem] trainer: dots {a['dots']} / twin {b['dots']}, projected {a['projected']}, grad norms {a['gn']} / twin {b['gn']}")
    assert a["projected"] == [0.0, 1.0, 1.0, 0.0] and b["projected"] == a["projected"]
    assert 1.0 in a["projected"] and 0.0 in a["projected"]
    assert len(a["loss"]) == 8 and len(a["gn"]) == 4
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert abs(x - y) <= 1e-6 * abs(y), f"micro-batch {i}: loss {x} vs {y}"
    for i, (x, y) in enumerate(zip(a["gn"], b["gn"])):
        assert abs(x - y) <= 1e-5 * abs(y), f"step {i}: grad norm {x} vs {y}"
    d = float((a["params"] - b["params"]).abs().max())
    print(f"[agem] trainer: parameters differ by {d:.3e} after 4 optimiser steps")
    assert d <= 1e-6, f"parameters differ by {d} after 4 optimiser steps"


def test_agem_bf16_overwrite_mode_equals_zero_then_accumulate():
    """accumulate = 2 in bf16 with ``dw_group_layers = 2``: the window's first sweep overwrites the weight-matrix gradients that the
    previous step's projection left behind.  Losses, the clip's gradient norms and the parameters after four optimiser steps equal the run
    that zeroes and accumulates (the bounds of tests/test_gpu_lwf.py::test_lwf_overwrite_mode_equals_zero_then_accumulate)."""
    from mafed_amd import AGEM
    a = _trainer_run(AGEM, torch.bfloat16, overwrite=True)
    b = _trainer_run(AGEM, torch.bfloat16, overwrite=False)
    print(f"[agem] bf16: projected {a['projected']} / {b['projected']}, dots {a['dots']}")
    assert 1.0 in a["projected"] and a["projected"] == b["projected"]
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), f"micro-batch {i}: loss {x} vs {y}"
    assert len(a["gn"]) == 4
    for i, (x, y) in enumerate(zip(a["gn"], b["gn"])):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), f"step {i}: grad norm {x} vs {y}"
    d = float((a["params"] - b["params"]).abs().max())
    assert d <= 2e-5, f"parameters differ by {d} after 4 optimiser steps"
    assert a["model"]._dw_stale and not b["model"]._dw_stale


def test_agem_refuses_a_reducer():
    from mafed_amd import Trainer
    cfg, sd, _, batch, _ = golden_setup("t64")
    model = _model(cfg, sd)
    agem = _agem(model, batch)
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, agem, _conf(), task_id=1, reducer=types.SimpleNamespace(world=2))   # a stub: refused before anything looks at it
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, agem, _conf(), task_id=1, ddp=True)
    Trainer(model, agem, _conf(), task_id=1)
