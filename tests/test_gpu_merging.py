"""TaskMerging (mafed_amd/methods/merging.py) on the tiny golden configuration, in fp32 and under the bf16 default
Trainer with the pipelined optimiser: training under it is Naive's bit for bit, the streaming state equals the numpy restatement
(tests/merge_ref.py) on the parameters snapshotted at ``begin`` and at every ``update``, ``merged_view`` holds the restatement's merged
model and takes it away again, and the refusals raise."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import golden_setup
from tests.merge_ref import MergeRef, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
RULES = ["sum", "magmax", "ties"]
DTYPES = [torch.float32, torch.bfloat16]
DENSITY, SCALING, TASKS, STEPS = 0.2, 0.3, 3, 3


def _model(cfg, sd, dtype=torch.float32):
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    mc = VLPythiaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        vision_hidden_size=cfg.vision_hidden_size, num_vision_tokens=cfg.num_vision_tokens)
    m = VLPythiaForCausalLM(mc, compute_dtype=dtype, device=DEV)
    m.load_state_dict(sd, strict=True)
    if dtype == torch.bfloat16:
        m.dw_group_layers = 2
    return m


def _to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _conf(lr=2e-3, grad_norm=2.0):
    return types.SimpleNamespace(accumulate_grad_batches=1, replay_interval=1, grad_norm=grad_norm, learning_rate=lr, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_steps=0, total_steps=100)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _host(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.detach().cpu().numpy()


def _probe(model, batch):
    """Eval-mode logits of a fixed batch."""
    was = model.training
    model.eval()
    with torch.no_grad():
        logits = model(**batch, return_dict=True).logits.clone()
    model.train(was)
    return logits


_RUNS = {}


def _train(dtype, rule=None, independent=False, control=False):
    """TASKS tasks of STEPS Trainer steps on t64 (pipelined optimiser, overwriting first sweep) under Naive (``rule`` None) or
    TaskMerging(rule).  -> dict(model, method, losses, norms, grads (in front of each clip), params (after each step), snapshots
    (flat_params at begin and at every update, in front of an ``independent`` reset)).  Run once per key and shared, read only."""
    key = (dtype, rule, independent, control)           # (control: a second run of the same thing)
    if key in _RUNS:
        return _RUNS[key]
    from mafed_amd import Naive, TaskMerging, Trainer
    from oracle import vlpythia_ref as R
    cfg, sd, _, _, _ = golden_setup("t64")
    model = _model(cfg, sd, dtype)
    method = Naive() if rule is None else TaskMerging(rule=rule, scaling=SCALING, density=DENSITY, independent=independent)
    out = dict(model=model, method=method, losses=[], norms=[], grads=[], params=[], snapshots=[model.flat_params.clone()], cfg=cfg, sd=sd)
    if rule is not None:
        method.begin(model)
    for t in range(TASKS):
        batches = [_to_dev(R.make_batch(cfg, 3, 6, seed=700 + 10 * t + i, pad=True, n_answer=3)) for i in range(STEPS)]
        tr = Trainer(model, method, _conf(), task_id=t, pipeline_optimizer=True, overwrite_weight_grads=True)
        clip = tr.optimizer.clip_grad_norm_

        def clip_and_record(*a, **kw):
            out["grads"].append(model.flat_grads.clone())
            return clip(*a, **kw)
        tr.optimizer.clip_grad_norm_ = clip_and_record
        for i, b in enumerate(batches):
            rec = tr.step(dict(b), i)
            tr.join()
            assert rec["stepped"]
            out["losses"].append(rec["loss"].reshape(()).clone())
            out["norms"].append(rec["grad_norm"].reshape(()).clone())
            out["params"].append(model.flat_params.clone())
        tr.optimizer.clip_grad_norm_ = clip
        out["snapshots"].append(model.flat_params.clone())
        if rule is not None:
            method.update(model)
            assert method.task_id == t + 1
    torch.cuda.synchronize()
    _RUNS[key] = out
    return out


def _segments(model):
    return [(o, n) for o, n, _ in model._offsets.values()]


def _oracle(run, rule, snapshots=None):
    ref = MergeRef(rule, density=DENSITY, segments=_segments(run["model"]))
    snaps = [_host(s) for s in (run["snapshots"] if snapshots is None else snapshots)]
    ref.begin(snaps[0])
    for s in snaps[1:]:
        ref.update(s)
    return ref


def _assert_state(tm, ref, rule):
    assert same_bits(_host(tm.base), ref.base)
    if rule == "ties":
        assert tm.acc is None
        for name in ("pos", "neg", "counts"):
            assert same_bits(_host(getattr(tm, name)), getattr(ref, name)), name
    else:
        assert tm.pos is None and tm.neg is None and tm.counts is None
        assert same_bits(_host(tm.acc), ref.acc)


WHAT = ("losses", "norms", "grads", "params", "snapshots")


def _first_difference(a, b):
    for what in WHAT:
        for i, (x, y) in enumerate(zip(a[what], b[what])):
            if not torch.equal(_bits(x), _bits(y)):
                return f"{what}[{i}]"
    return None


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_training_under_taskmerging_is_naive(dtype, monkeypatch):
    """Losses, logged norms, gradients in front of every clip, parameters behind every step and at every task boundary: Naive's bit for
    bit.  The bf16 step sums its bias and embedding gradients with fp32 atomics, so there two runs of Naive
    itself need not agree: a second Naive run is the control, the comparison is made whenever the control reproduces the first run, and
    in every case one step under each method must consist of the same launches with the same work, none of them a merge pass."""
    import collections
    from mafed_amd import Naive, TaskMerging, Trainer, ops
    from mafed_amd.profiler import KernelProfile
    naive = _train(dtype)
    merged = _train(dtype, "magmax")
    assert len(naive["grads"]) == TASKS * STEPS == len(merged["grads"]) == len(naive["losses"])
    assert not torch.equal(naive["snapshots"][0], naive["snapshots"][1]) and bool(naive["grads"][0].any())
    control = None if dtype == torch.float32 else _first_difference(_train(dtype, control=True), naive)
    diff = _first_difference(merged, naive)
    print(f"[merge] {dtype}: first difference from Naive: {diff}; between two Naive runs: {control}")
    if control is None:
        assert diff is None, f"{diff} differs from Naive's"
    # no hook launches anything: one step under each method, every merge pass forbidden, the library's own launch records compared
    for name in ("merge_fold_", "merge_ties_fold_", "merge_apply_"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("TaskMerging launched a pass inside a step"))
    cfg, sd, _, batch, _ = golden_setup("t64")
    launches = []
    for method in (Naive(), TaskMerging(rule="ties")):
        model = _model(cfg, sd, dtype)
        if isinstance(method, TaskMerging):
            assert method.grads_only_through_model is True and method.single_process_only is False
            method.begin(model)
        tr = Trainer(model, method, _conf(), task_id=0, pipeline_optimizer=True, overwrite_weight_grads=True)
        with KernelProfile() as prof:
            tr.step(_to_dev(batch), 0)
            tr.join()
        launches.append(collections.Counter((tag, work) for tag, work, _ in prof.records()))
    assert launches[0] == launches[1] and sum(launches[0].values()) > 20
    assert not any(tag == "merge" for tag, _ in launches[1])


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_state_and_merged_view_equal_the_restatement(dtype, rule):
    run = _train(dtype, rule)
    model, tm = run["model"], run["method"]
    ref = _oracle(run, rule)
    _assert_state(tm, ref, rule)
    named = tm.named(model, "pos" if rule == "ties" else "acc")
    assert set(named) == set(model._offsets) and named.flat.data_ptr() == (tm.pos if rule == "ties" else tm.acc).data_ptr()
    if rule == "ties":
        report = tm.trim_report(model)
        assert list(report) == list(model._offsets)
        for (name, row), want in zip(report.items(), ref.stats):
            assert [row["m"], row["r"], row["kept"], row["tau_bits"]] == want.tolist(), name
            assert row["m"] == model._offsets[name][1]
        assert bool((tm.counts.sum(1) >= 2).any())
    else:
        assert tm.trim_report(model) == {}
    cfg, sd, _, probe, _ = golden_setup("t64")
    probe = _to_dev(probe)
    with_shadow = model.flat_shadow is not None
    assert with_shadow == (dtype == torch.bfloat16)
    p0 = model.flat_params.clone()
    sh0 = model.flat_shadow.clone() if with_shadow else None
    before = _probe(model, probe)
    twin = _model(cfg, sd, dtype)
    for scaling in (None, 1.0):
        want_p, want_sh = ref.merged(SCALING if scaling is None else scaling, shadow=with_shadow)
        with tm.merged_view(model, scaling) as m:
            assert m is model
            assert same_bits(_host(model.flat_params), want_p), f"scaling {scaling}: the view's parameters"
            if with_shadow:
                assert same_bits(_host(model.flat_shadow), want_sh), f"scaling {scaling}: the view's shadow"
            logits = _probe(model, probe)
        with torch.no_grad():
            twin.flat_params.copy_(torch.from_numpy(want_p).to(DEV))
        twin.sync_shadow()
        assert torch.equal(_bits(logits), _bits(_probe(twin, probe))), f"scaling {scaling}: logits of the view against a model loaded with the restatement"
        assert not torch.equal(logits, before)
        assert torch.equal(_bits(model.flat_params), _bits(p0))                 # leaving the view puts everything back
        if with_shadow:
            assert torch.equal(_bits(model.flat_shadow), _bits(sh0))
        assert torch.equal(_bits(_probe(model, probe)), _bits(before))
    assert not np.array_equal(want_p, _host(p0))


@pytest.mark.parametrize("rule", ["magmax", "ties"])
def test_independent_puts_base_back_and_merge_writes_for_good(rule):
    from mafed_amd import ops
    run = _train(torch.bfloat16, rule, independent=True)
    model, tm = run["model"], run["method"]
    assert torch.equal(_bits(model.flat_params), _bits(tm.base))                # after the last update
    assert torch.equal(_bits(model.flat_shadow), _bits(ops.cast(tm.base, torch.bfloat16)))
    ref = _oracle(run, rule)
    _assert_state(tm, ref, rule)
    want_p, want_sh = ref.merged(SCALING, shadow=True)
    tm.merge_(model)
    assert same_bits(_host(model.flat_params), want_p) and same_bits(_host(model.flat_shadow), want_sh)
    with torch.no_grad():                                                       # (the run is shared: leave it as update left it)
        model.flat_params.copy_(tm.base)
    model.sync_shadow()


@pytest.mark.parametrize("rule", RULES)
def test_state_dict_round_trip_through_the_host(rule):
    from mafed_amd import TaskMerging
    run = _train(torch.float32, rule)
    model, tm = run["model"], run["method"]
    sd = tm.state_dict()
    assert set(sd) == {"base", "acc", "pos", "neg", "counts", "task_id", "rule", "density"}
    assert sd["task_id"] == TASKS and sd["rule"] == rule and sd["density"] == DENSITY
    tm2 = TaskMerging(rule="sum" if rule != "sum" else "ties", density=0.9, scaling=SCALING)
    tm2.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()})    # as a checkpoint read on the host gives it
    assert tm2.rule == rule and tm2.density == DENSITY and tm2.task_id == TASKS
    for name in ("base", "acc", "pos", "neg", "counts"):
        a, b = getattr(tm, name), getattr(tm2, name)
        assert (a is None) == (b is None)
        if a is not None:
            assert b.data_ptr() != a.data_ptr() and torch.equal(a.cpu(), b.cpu()) and same_bits(_host(a), _host(b))
    with tm.merged_view(model):
        want = model.flat_params.clone()
    with tm2.merged_view(model):                        # the loaded state moves to the model's device at its first use
        assert torch.equal(_bits(model.flat_params), _bits(want))
    for key in sd:
        with pytest.raises(ValueError, match=key):
            tm2.load_state_dict({k: v for k, v in sd.items() if k != key})


def test_refusals():
    from mafed_amd import CLMethod, TaskMerging, Trainer
    assert "merging" not in CLMethod.names()
    for bad in ("mean", "", None):
        with pytest.raises(ValueError, match="rule"):
            TaskMerging(rule=bad)
    for bad in (0.0, -0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match="density"):
            TaskMerging(density=bad)
    TaskMerging(density=1.0)
    cfg, sd, _, batch, _ = golden_setup("t64")
    batch = _to_dev(batch)
    model = _model(cfg, sd)
    foreign = torch.nn.Linear(2, 2).to(DEV)
    tm = TaskMerging(rule="ties")

    def enter(m, plugin=tm):
        with plugin.merged_view(m):
            pass
    for call in (lambda: tm.begin(foreign), lambda: tm.update(foreign), lambda: enter(foreign), lambda: tm.merge_(foreign),
                 lambda: tm.named(foreign), lambda: tm.trim_report(foreign)):
        with pytest.raises(TypeError, match="native model"):
            call()
    for call in (lambda: tm.update(model), lambda: enter(model), lambda: tm.merge_(model), lambda: tm.named(model)):
        with pytest.raises(RuntimeError, match="begin"):
            call()                                      # nothing works before begin
    tm.begin(model)
    with pytest.raises(RuntimeError, match="already"):
        tm.begin(model)                                 # a second begin
    with pytest.raises(KeyError):
        tm.named(model, "owner")
    with pytest.raises(RuntimeError, match="no acc"):
        tm.named(model, "acc")                          # the ties rule has no acc
    tr = Trainer(model, tm, _conf())
    tr.step(dict(batch), 0)
    tr.join()
    p0 = model.flat_params.clone()
    with tm.merged_view(model):                         # before the first update the view is base itself
        assert torch.equal(_bits(model.flat_params), _bits(tm.base)) and not torch.equal(model.flat_params, p0)
        with pytest.raises(RuntimeError, match="merged_view"):
            tr.step(dict(batch), 1)                     # a step inside a view
        with pytest.raises(RuntimeError, match="nest"):
            enter(model)                                # a nested view
        with pytest.raises(RuntimeError, match="merged_view"):
            tm.update(model)                            # an update inside a view
        with pytest.raises(RuntimeError, match="merged_view"):
            tm.merge_(model)
    tr.join()
    assert torch.equal(_bits(model.flat_params), _bits(p0)) and tm.task_id == 0
    model.zero_grad()
    tm.task_id = 255                                    # the byte counters hold 255 folds
    pos = tm.pos.clone()
    with pytest.raises(RuntimeError, match="255 tasks"):
        tm.update(model)
    assert tm.task_id == 255 and torch.equal(tm.pos, pos)
    other = _model(*golden_setup("m64")[:2])
    if other.flat_params.numel() != model.flat_params.numel():
        with pytest.raises(ValueError, match="another model"):
            tm.update(other)
