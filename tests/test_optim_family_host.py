"""CPU: FlatAdam / FlatAdamax (the reference's optim = "adam" / "adamax") -- exports, torch defaults, torch state names, state_dict
round trip and refusal, the Trainer's optimiser choice, and which launches the flat passes make (the ops call recorded, no GPU)."""
import inspect
import types

import pytest
import torch


class _FlatModel:
    """Stand-in with the two attributes the optimiser constructor reads (decayed segment = the first 12 elements)."""

    def __init__(self, n=20, n_decay=12):
        self.flat_params = torch.arange(n, dtype=torch.float32)
        self.flat_grads = torch.ones(n)
        self.flat_shadow = None
        self._n_decay = n_decay

    def decay_split(self):
        return self._n_decay


def _default(fn, name):
    return inspect.signature(fn).parameters[name].default


def test_classes_are_exported():
    import mafed_amd
    from mafed_amd.optim import FlatAdam, FlatAdamax, FlatAdamW
    assert mafed_amd.FlatAdam is FlatAdam and mafed_amd.FlatAdamax is FlatAdamax and mafed_amd.FlatAdamW is FlatAdamW


@pytest.mark.parametrize("ours,theirs", [("FlatAdam", torch.optim.Adam), ("FlatAdamax", torch.optim.Adamax)])
def test_defaults_are_torch_defaults(ours, theirs):
    from mafed_amd import optim
    cls = getattr(optim, ours)
    for name in ("lr", "betas", "eps", "weight_decay"):
        assert _default(cls.__init__, name) == _default(theirs.__init__, name), name
    assert _default(cls.__init__, "eps") == 1e-8
    opt = cls(_FlatModel())
    assert opt.betas == tuple(_default(theirs.__init__, "betas")) and opt.eps == 1e-8 and opt.weight_decay == 0


@pytest.mark.parametrize("name,keys", [("FlatAdamW", ("exp_avg", "exp_avg_sq")), ("FlatAdam", ("exp_avg", "exp_avg_sq")),
                                       ("FlatAdamax", ("exp_avg", "exp_inf"))])
def test_state_names_follow_torch(name, keys):
    from mafed_amd import optim
    model = _FlatModel()
    opt = getattr(optim, name)(model)
    assert opt.STATE == keys
    for k in keys:
        buf = getattr(opt, k)
        assert buf.shape == model.flat_params.shape and buf.dtype == torch.float32 and float(buf.abs().sum()) == 0.0
    sd = opt.state_dict()
    assert set(sd) == set(keys) | {"optim", "step", "sched"}
    assert sd["optim"] == {"FlatAdamW": "adamw", "FlatAdam": "adam", "FlatAdamax": "adamax"}[name]


def test_state_dict_round_trip_and_refusal():
    from mafed_amd.optim import FlatAdam, FlatAdamax, FlatAdamW
    a = FlatAdamax(_FlatModel())
    a.exp_avg.uniform_()
    a.exp_inf.uniform_()
    a.step_count = 7
    a.attach_schedule(2, 30)
    sd = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in a.state_dict().items()}
    b = FlatAdamax(_FlatModel())
    b.load_state_dict(sd)
    assert torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_inf, a.exp_inf)
    assert b.step_count == 7 and int(b.state_dev) == 7 and b._sched == (2, 30)
    # another optimiser's state is refused, whatever the overlap of buffer names
    with pytest.raises(ValueError, match="adamw"):
        FlatAdam(_FlatModel()).load_state_dict(FlatAdamW(_FlatModel()).state_dict())
    with pytest.raises(ValueError, match="adamax"):
        FlatAdam(_FlatModel()).load_state_dict(sd)
    with pytest.raises(ValueError, match="adam"):
        FlatAdamW(_FlatModel()).load_state_dict(FlatAdam(_FlatModel()).state_dict())
    # AdamW state saved before the tag existed still loads into AdamW
    w = FlatAdamW(_FlatModel())
    legacy = {"exp_avg": torch.full((20,), 2.0), "exp_avg_sq": torch.full((20,), 3.0), "step": 4, "sched": (1, 10)}
    w.load_state_dict(legacy)
    assert float(w.exp_avg_sq[0]) == 3.0 and w.step_count == 4


def test_trainer_optimiser_choice(monkeypatch):
    from mafed_amd import trainer as T
    from mafed_amd.optim import FlatAdam, FlatAdamax, FlatAdamW
    assert T._OPTIMIZERS == {"adamw": FlatAdamW, "adam": FlatAdam, "adamax": FlatAdamax}
    for bad in ("sgd", "AdamW", ""):
        with pytest.raises(ValueError, match="invalid optimizer"):
            T.Trainer(_FlatModel(), types.SimpleNamespace(), types.SimpleNamespace(optim=bad))
    # what the Trainer passes: lr, betas and the decayed segment's weight decay; eps only when configured
    seen = {}

    class Stop(Exception):
        pass

    def fake(name):
        def ctor(model, **kw):
            seen[name] = kw
            raise Stop
        return ctor

    monkeypatch.setattr(T, "_OPTIMIZERS", {k: fake(k) for k in ("adamw", "adam", "adamax")})
    for name in ("adam", "adamax"):
        with pytest.raises(Stop):
            T.Trainer(_FlatModel(), None, types.SimpleNamespace(optim=name, learning_rate=3e-4, betas=(0.8, 0.9), weight_decay=0.02))
        assert seen[name] == {"lr": 3e-4, "betas": (0.8, 0.9), "weight_decay": 0.02}
    with pytest.raises(Stop):
        T.Trainer(_FlatModel(), None, types.SimpleNamespace(optim="adam", eps=1e-7))
    assert seen["adam"]["eps"] == 1e-7
    with pytest.raises(Stop):
        T.Trainer(_FlatModel(), None, types.SimpleNamespace())   # no optim in the config: AdamW, as before
    assert "adamw" in seen and "eps" not in seen["adamw"]


@pytest.mark.parametrize("name,rule,second", [("FlatAdam", "adam", "exp_avg_sq"), ("FlatAdamax", "adamax", "exp_inf")])
def test_apply_launches_the_rule_per_segment(monkeypatch, name, rule, second):
    from mafed_amd import ops, optim
    calls = []
    monkeypatch.setattr(ops, "adam_family_step_", lambda *a, **kw: calls.append((a, kw)))
    monkeypatch.setattr(ops, "adamw_step_", lambda *a, **kw: pytest.fail("AdamW kernel launched for " + name))
    model = _FlatModel()
    opt = getattr(optim, name)(model, weight_decay=0.1)
    for zero in (False, True):
        calls.clear()
        opt.apply(grad_mul=0.5, zero_grads=zero)
        assert len(calls) == 2
        for (a, kw), (lo, hi, wd) in zip(calls, [(0, 12, 0.1), (12, 20, 0.0)]):
            assert a[0] == rule
            assert a[1].data_ptr() == model.flat_params[lo:].data_ptr() and a[1].numel() == hi - lo
            assert a[4].data_ptr() == getattr(opt, second)[lo:].data_ptr()
            assert a[9] == wd and a[12] == 0.5
            assert kw["zero_n"] == ((hi - lo) if zero else 0)
