"""CPU: the float64 yardstick of GEM's projection (tests/gem_ref.py) -- the enumeration solve against an independent KKT checker and an
independent projected-gradient solver --, the preconditions of the GPU cases, and the plugin's place in the package."""
import types

import numpy as np
import pytest

from tests import gem_ref as G
from tests.agem_ref import agem_project


def _vectors(seed, K, n=4097):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), [rng.standard_normal(n) for _ in range(K)]


@pytest.mark.parametrize("K", range(1, 9))
def test_enumeration_vs_kkt_and_projected_gradient(K):
    """Random SPD problems with a known support.  At condition number 1e3 the accelerated projected gradient converges (it stops when an
    iteration moves u by 1e-13 max|u|; the distance to the optimum is then below 1e-13 times the condition number, checked at 1e-8);
    at 1e6 it would need millions of iterations, so there only the KKT checker judges: residuals of a float64 Cholesky solve, at most
    a few ulps of the terms they are sums of (1e-12 leaves three digits)."""
    for seed in range(6):
        for cond, margin in ((1e3, 0.0), (1e3, 0.5), (1e6, 0.0), (1e6, 0.5)):
            gram, active = G.spd_problem(K, seed, cond=cond, margin=margin)
            s = G.gem_solve(gram, margin, 0.0)
            if not s["violated"]:
                assert (s["q"] >= 0).all() and not s["v"].any()
                continue
            assert [k for k in range(K) if s["mask"] >> k & 1] == active and s["support"] == len(active)
            assert (s["v"] >= margin).all()
            res = G.kkt_residuals(s["P"], s["qp"], s["u"])
            assert max(res) <= 1e-12, (K, seed, cond, margin, res)
            assert G.decision_gap(gram, margin, 0.0) >= 1e-2
            if cond == 1e3:
                u = G.pgd_solve(s["P"], s["qp"])
                assert np.abs(u - s["u"]).max() <= 1e-8 * np.abs(s["u"]).max(), (K, seed, margin, u, s["u"])


def test_kkt_checker_sees_a_wrong_answer():
    gram, active = G.spd_problem(4, 1, cond=1e3, active=[0, 2])
    s = G.gem_solve(gram, 0.0, 0.0)
    assert max(G.kkt_residuals(s["P"], s["qp"], s["u"])) <= 1e-12
    wrong = s["u"].copy()
    wrong[0] *= 1.0 + 1e-6
    assert max(G.kkt_residuals(s["P"], s["qp"], wrong)) > 1e-8
    wrong = s["u"].copy()
    wrong[1] = 1e-3                      # a constraint that should be off the support
    assert max(G.kkt_residuals(s["P"], s["qp"], wrong)) > 1e-8
    assert G.kkt_residuals(s["P"], s["qp"], -s["u"])[0] == 1.0


@pytest.mark.parametrize("K", range(1, 9))
def test_projected_gradient_satisfies_every_constraint(K):
    """margin = 0, eps = 0: g~ . r_k >= -1e-12 sum|g r_k| for every k, whichever constraints were violated."""
    for seed in range(4):
        g, refs = _vectors(10 * K + seed, K)
        refs = [r if np.dot(g, r) > 0 and j % 2 else -np.sign(np.dot(g, r)) * r for j, r in enumerate(refs)]   # at least ref 0 opposes g
        gram, sabs = G.gem_gram(g, refs)
        s = G.gem_solve(gram, 0.0, 0.0)
        assert s["violated"] and s["support"] >= 1
        gt = G.gem_project(g, refs, s["v"], True)
        for k, r in enumerate(refs):
            scale = sabs[0, k + 1] + sum(abs(s["v"][j]) * sabs[j + 1, k + 1] for j in range(K))
            assert np.dot(gt, r) >= -1e-12 * scale, (K, seed, k)
        assert np.dot(gt, gt) < np.dot(g, g)


def test_not_violated_is_the_identity():
    g, refs = _vectors(3, 3)
    refs = [np.sign(np.dot(g, r)) * r for r in refs]
    g[5] = -0.0
    s = G.gem_solve(G.gem_gram(g, refs)[0], 0.5, 1e-3)
    assert not s["violated"] and not s["v"].any() and s["support"] == 0
    assert G.gem_project(g, refs, s["v"], False).tobytes() == g.tobytes()
    # orthogonal (q_k == 0 exactly) is not a violation either
    e = np.eye(3)
    assert not G.gem_solve(G.gem_gram(e[0], [e[1], e[2]])[0], 0.5, 1e-3)["violated"]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_one_constraint_without_margin_is_agem(seed):
    g, (r,) = _vectors(seed, 1)
    if np.dot(g, r) >= 0:
        r = -r
    want, (dot, rsq, alpha, violated, _) = agem_project(g, r)
    s = G.gem_solve(G.gem_gram(g, [r])[0], 0.0, 0.0)
    assert violated and s["violated"] and s["mask"] == 1
    gram = G.gem_gram(g, [r])[0]
    assert abs(s["v"][0] + gram[0, 1] / gram[1, 1]) <= 8 * 2.0 ** -53 * abs(alpha)   # sqrt, two divisions and a negation against one division
    # (against agem_ref's own sums, which add the 4097 products in another order: n 2^-53 sum|g r| / |dot| <= 1e-10 here)
    assert abs(s["v"][0] + alpha) <= 1e-10 * abs(alpha)
    np.testing.assert_allclose(G.gem_project(g, [r], s["v"], True), want, rtol=0, atol=1e-10 * abs(alpha) * np.abs(r).max())
    # K = 1 closed form with margin and eps
    s = G.gem_solve(G.gem_gram(g, [r])[0], 0.5, 1e-3)
    assert abs(s["v"][0] - max(0.5, -dot / (rsq + 1e-3))) <= 1e-15


def test_diagonal_problem_closed_form():
    P = np.diag([1.0, 4.0, 0.25, 9.0])
    q = np.array([-3.0, 2.0, -0.05, -1.0])
    gram = np.zeros((5, 5))
    gram[1:, 1:], gram[0, 1:], gram[1:, 0], gram[0, 0] = P, q, q, 20.0
    for margin, eps in ((0.0, 0.0), (0.5, 1e-3)):
        s = G.gem_solve(gram, margin, eps)
        np.testing.assert_allclose(s["v"], np.maximum(margin, -q / (P.diagonal() + eps)), rtol=1e-15, atol=0)


def test_duplicate_references_without_eps():
    """r_1 = r_2 and eps = 0: P is singular, the supports {1} and {2} tie exactly (the lower mask wins), {1, 2} is skipped at its second
    pivot.  The KKT conditions hold and G'v is the eps -> 0 limit's."""
    g, (r, r3) = _vectors(21, 2)
    if np.dot(g, r) >= 0:
        r = -r
    refs = [r, r.copy(), r3]
    gram, _ = G.gem_gram(g, refs)
    s = G.gem_solve(gram, 0.0, 0.0)
    assert s["violated"] and s["mask"] & 0b11 == 0b01
    assert max(G.kkt_residuals(s["P"], s["qp"], s["u"])) <= 1e-12
    lim = G.gem_solve(gram, 0.0, 1e-9 * gram[1, 1])
    assert lim["mask"] & 0b11 == 0b11   # (the limit spreads the coefficient over both copies; P_SS has condition number 1e9 there)
    a, b = (sum(v * x for v, x in zip(sol["v"], refs)) for sol in (s, lim))
    assert np.abs(a - b).max() <= 1e-8 * np.abs(b).max()


def test_non_finite_gram_poisons():
    gram, _ = G.spd_problem(3, 0)
    gram[1, 2] = gram[2, 1] = np.nan
    s = G.gem_solve(gram, 0.5, 1e-3)
    assert s["violated"] and np.isnan(s["v"]).all()


def test_gpu_solve_suite_decides_clearly():
    """Every problem of tests/test_gpu_gem_kernels.py's solve suite: the expected support is the oracle's, its decision is at least 1e-2
    of its scale away from flipping (the feasibility tolerances are 1e-9), and no other support passes the feasibility tests.  Supports
    of every size occur, K = 8 with all eight included."""
    sizes = set()
    for K, seed, margin, gram, active in G.solve_suite():
        s = G.gem_solve(gram, margin, 0.0)
        assert s["violated"], (K, seed)
        assert [k for k in range(K) if s["mask"] >> k & 1] == active
        assert G.decision_gap(gram, margin, 0.0) >= 1e-2, (K, seed)
        assert sum(1 for c in G.enumerate_supports(s["P"], s["qp"]) if c[4]) == 1, (K, seed)
        assert np.linalg.cond(s["P"]) <= 1.001e6
        sizes.add((K, len(active)))
    assert sizes >= {(K, n) for K in range(2, 9) for n in range(K + 1)} and (8, 8) in sizes


@pytest.mark.parametrize("key", list(G.ORACLE_CASES))
def test_gpu_case_preconditions_from_the_oracle(key):
    """The memory batches of tests/test_gpu_gem.py give the decision they are named for, clear of rounding: every |q_k| >= 1e-2
    sum|g r_k| and the chosen support at least 0.5 of its scale away from the next."""
    name, seeds, margin = key
    case = G.oracle_case(name, seeds, margin)
    s, gram, sabs = case["solve"], case["gram"], case["sabs"]
    print(f"[gem] {key}: q / sum|g r| {gram[0, 1:] / sabs[0, 1:]}, v {s['v']}, mask {s['mask']}")
    violated, support = G.ORACLE_CASES[key]
    assert (s["violated"], s["support"]) == (violated, support)
    assert (np.abs(gram[0, 1:]) >= 1e-2 * sabs[0, 1:]).all()
    if violated:
        assert G.decision_gap(gram, margin, 1e-3) >= 0.5
        assert max(G.kkt_residuals(s["P"], s["qp"], s["u"])) <= 1e-12


def test_trainer_case_gives_the_recorded_pattern():
    """The four optimiser steps of tests/test_gpu_gem.py's Trainer test along the float64 trajectory: one window with a strict subset of
    the constraints in the support, two with both, one that is not violated -- each clear of rounding."""
    steps = G.gem_trainer_fp64()
    for st in steps:
        s = st["solve"]
        print(f"[gem] trainer step: q / sum|g r| {st['gram'][0, 1:] / st['sabs'][0, 1:]}, v {s['v']}, mask {s['mask']}, norm {st['grad_norm']:.6g}")
    assert [(st["solve"]["violated"], st["solve"]["mask"]) for st in steps] == G.GEM_TRAINER_PATTERN
    pattern = G.GEM_TRAINER_PATTERN
    assert any(not v for v, _ in pattern) and any(v and m in (0b01, 0b10) for v, m in pattern) and any(m == 0b11 for _, m in pattern)
    for st in steps:
        assert (np.abs(st["gram"][0, 1:]) >= 1e-2 * st["sabs"][0, 1:]).all()
        if st["solve"]["violated"]:
            assert G.decision_gap(st["gram"], G.GEM_TRAINER["margin"], G.GEM_TRAINER["eps"]) >= 0.1


def _samples(n, T=5, lo=1, hi=50, seed=0):
    import torch
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(lo, hi, (n, T), generator=gen)
    return {"input_ids": ids, "attention_mask": torch.ones(n, T, dtype=torch.int64), "labels": ids.clone(),
            "patch_embeddings": torch.randn(n, 2, 4, generator=gen)}


def test_gem_is_exported_and_not_registered():
    import torch
    import mafed_amd
    from mafed_amd import CLMethod, GEM, Trainer
    from mafed_amd.methods import ER, CLStrategy, GEM as GEM2, LwF
    assert GEM is GEM2 and mafed_amd.methods.gem.GEM is GEM
    assert issubclass(GEM, ER) and issubclass(GEM, CLStrategy)
    assert "gem" not in CLMethod and CLMethod.extensions == {"lwf": LwF}
    opts = types.SimpleNamespace(tasks=["a", "b"], seed=0, batch_size=2)
    m = GEM(opts, memory_size=4, model_type="vlpythia")
    assert (m.margin, m.eps) == (0.5, 1e-3)
    assert m.replay(None) == (None, 0) and m.compute_loss(None, 1.5) == 1.5
    assert m.grads_only_through_model is False and m.single_process_only is True
    assert m.task_id == 0 and m.task_memories == [] and m.last_coef is None and m.last_gram is None
    m.update_after_backward(model=None)   # task 0: nothing, not even a look at the model
    with pytest.raises(TypeError, match="native model"):
        m.update({}, model=torch.nn.Linear(2, 2))
    with pytest.raises(ValueError):
        GEM(opts, memory_size=4, model_type="vlpythia", margin=-1.0)
    with pytest.raises(ValueError, match="single-process"):
        Trainer(types.SimpleNamespace(), m, reducer=object())
    with pytest.raises(ValueError, match="single-process"):
        Trainer(types.SimpleNamespace(), m, ddp=True)


def test_update_keeps_ers_selection_and_one_memory_per_task():
    """``update`` is ER's (same rng stream, same stored samples) plus one buffer per task over that task's samples, seeded opts.seed + 1 +
    task index; a ninth task is refused before anything has changed."""
    import torch
    from mafed_amd import ER, GEM
    opts = types.SimpleNamespace(tasks=[str(i) for i in range(11)], seed=5, batch_size=3)
    er, gem = ER(opts, memory_size=40, model_type="vlpythia"), GEM(opts, memory_size=40, model_type="vlpythia")
    for t in range(8):
        data = _samples(10, lo=100 * t + 1, hi=100 * t + 50, seed=t)
        er.update(dict(data))
        gem.update(dict(data))
        assert len(gem.task_memories) == t + 1 == gem.task_id and len(gem.task_memories[t]) == 4
        assert torch.equal(gem.datasets[t]["input_ids"], er.datasets[t]["input_ids"])
        assert torch.equal(gem.task_memories[t].data["input_ids"], er.datasets[t]["input_ids"])
        assert gem.task_memories[t].gen.initial_seed() == 5 + 1 + t
    for k in er.mem_dataloader.data:
        assert torch.equal(gem.mem_dataloader.data[k], er.mem_dataloader.data[k])
    for t, mem in enumerate(gem.task_memories):   # disjoint token ids per task: every draw stays inside its own task
        ids = next(iter(mem))["input_ids"]
        assert int(ids.min()) > 100 * t and int(ids.max()) < 100 * t + 50
    before = (gem.task_id, len(gem.datasets), len(gem.mem_dataloader), gem.rng.bit_generator.state)
    with pytest.raises(RuntimeError, match="GEM_MAX_REFS"):
        gem.update(_samples(10, seed=99))
    assert before == (gem.task_id, len(gem.datasets), len(gem.mem_dataloader), gem.rng.bit_generator.state)
