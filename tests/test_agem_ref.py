"""CPU: the float64 yardstick of the A-GEM projection (tests/agem_ref.py), the preconditions of the GPU cases from the whole-step oracle,
and the plugin's place in the package."""
import numpy as np
import pytest

from tests.agem_ref import ORACLE_CASES, agem_project, agem_stats, oracle_case


def _pair(seed, n=4097):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(n)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_projection_removes_the_component_along_r_when_violated(seed):
    g, r = _pair(seed)
    if np.dot(g, r) >= 0:
        r = -r
    gp, (dot, rsq, alpha, violated, sabs) = agem_project(g, r)
    assert violated and dot < 0 and alpha == dot / rsq
    assert abs(np.dot(gp, r)) <= 1e-12 * sabs
    # the correction is along r only, and shortens g
    assert np.dot(gp, gp) < np.dot(g, g)
    np.testing.assert_allclose(gp - g, -alpha * r, rtol=0, atol=1e-15 * np.abs(g).max())


def test_strongly_opposed_reference():
    g, _ = _pair(7)
    r = -g + 1e-3 * _pair(8)[1]
    gp, (dot, rsq, alpha, violated, sabs) = agem_project(g, r)
    assert violated and abs(alpha + 1.0) < 1e-2
    assert abs(np.dot(gp, r)) <= 1e-12 * sabs


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_projection_is_the_identity_without_a_violation(seed):
    g, r = _pair(seed)
    if np.dot(g, r) < 0:
        r = -r
    g[5] = -0.0
    gp, st = agem_project(g, r)
    assert not st[3] and st[2] == 0.0
    assert gp.tobytes() == np.asarray(g, np.float64).tobytes()
    # orthogonal (dot == 0 exactly) is not a violation either
    e0, e1 = np.eye(2)
    assert agem_stats(e0, e1)[2:4] == (0.0, False)


def test_zero_reference_is_the_identity():
    g, _ = _pair(11)
    gp, (dot, rsq, alpha, violated, _) = agem_project(g, np.zeros_like(g))
    assert (dot, rsq, alpha, violated) == (0.0, 0.0, 0.0, False)
    assert gp.tobytes() == g.tobytes()
    # rsq == 0 with a negative "dot" cannot happen; the rule still guards the division
    assert agem_stats(np.zeros(0), np.zeros(0))[:4] == (0.0, 0.0, 0.0, False)


# dot, dot / sum|g r| and alpha of the whole-step oracle (tests.helpers.step_fp64 on the golden weights), to the digits given
EXPECTED = {("t64", 902): (-7.907, -0.138, -0.0898), ("t128", 901): (-11.054, -0.095, -0.0548), ("t128", 903): (9.242, 0.056, 0.0),
            ("t64", "self"): (156.66, 1.0, 0.0)}
DOT_ATOL = {("t64", "self"): 1e-2}   # one unit of the last digit given; 1e-3 for the others


@pytest.mark.parametrize("name,seed", list(ORACLE_CASES))
def test_gpu_case_preconditions_from_the_oracle(name, seed):
    """The memory batches of tests/test_gpu_agem.py give the sign they are named for, clear of rounding: |dot| >= 1e-2 sum|g r|."""
    dot, rsq, alpha, violated, sabs = oracle_case(name, seed)["stats"]
    print(f"[agem] {name} / {seed}: dot {dot:.6g}, dot / sum|g r| {dot / sabs:.4g}, rsq {rsq:.6g}, alpha {alpha:.6g}")
    sign = ORACLE_CASES[(name, seed)]
    assert (dot < 0) == (sign < 0) and violated == (sign < 0)
    assert abs(dot) >= 1e-2 * sabs
    e_dot, e_ratio, e_alpha = EXPECTED[(name, seed)]
    assert abs(dot - e_dot) <= DOT_ATOL.get((name, seed), 1e-3)
    assert abs(dot / sabs - e_ratio) <= 1e-3 and abs(alpha - e_alpha) <= 1e-4
    if seed == "self":
        assert dot == rsq == sabs   # ||g||^2


def test_trainer_case_projects_on_some_steps_and_not_on_others():
    """The four optimiser steps of tests/test_gpu_agem.py::test_agem_trainer_matches_torch_double along the float64 trajectory: dots
    +2.651, -1.637, -0.874, +1.208, each at least 0.13 sum|g r| away from zero."""
    from tests.agem_ref import agem_trainer_fp64
    stats = agem_trainer_fp64()
    for st in stats:
        print("[agem] trainer step: dot %.6g, rsq %.6g, alpha %.6g, dot / sum|g r| %.4f" % (st[0], st[1], st[2], st[0] / st[4]))
    assert [st[3] for st in stats] == [False, True, True, False]
    assert all(abs(st[0]) >= 0.1 * st[4] for st in stats)
    np.testing.assert_allclose([st[0] for st in stats], [2.651, -1.637, -0.874, 1.208], atol=1e-3)


def test_agem_is_exported_and_not_registered():
    import mafed_amd
    from mafed_amd import AGEM, CLMethod
    from mafed_amd.methods import AGEM as AGEM2, ER, CLStrategy, LwF
    assert AGEM is AGEM2 and mafed_amd.methods.agem.AGEM is AGEM
    assert issubclass(AGEM, ER) and issubclass(AGEM, CLStrategy)
    assert "agem" not in CLMethod and CLMethod.extensions == {"lwf": LwF}
    assert set(CLMethod) == {"naive", "ewc", "replay", "featdistill"}
    import types
    opts = types.SimpleNamespace(tasks=["a", "b"], seed=0, batch_size=2)
    m = AGEM(opts, memory_size=4, model_type="vlpythia")
    assert m.replay(None) == (None, 0)
    assert m.grads_only_through_model is False and m.single_process_only is True
    assert m.task_id == 0 and m.mem_dataloader is None and m.last_alpha is None
    assert m.compute_loss(None, 1.5) == 1.5
    m.update_after_backward(model=None)   # task 0: nothing, not even a look at the model
    import torch
    with pytest.raises(TypeError, match="native model"):   # a foreign nn.Module, as LwF
        m.update({}, model=torch.nn.Linear(2, 2))
    m.task_id, m.mem_dataloader = 1, [0]
    with pytest.raises(TypeError, match="native model"):
        m.update_after_backward(model=torch.nn.Linear(2, 2))


def test_trainer_refuses_a_reducer_for_a_single_process_plugin():
    """The guard sits in front of everything that needs a GPU: a stub model is enough."""
    import types
    from mafed_amd import AGEM, Trainer
    opts = types.SimpleNamespace(tasks=["a", "b"], seed=0, batch_size=2)
    with pytest.raises(ValueError, match="single-process"):
        Trainer(types.SimpleNamespace(), AGEM(opts, memory_size=4, model_type="vlpythia"), reducer=object())
    with pytest.raises(ValueError, match="single-process"):
        Trainer(types.SimpleNamespace(), AGEM(opts, memory_size=4, model_type="vlpythia"), ddp=True)
