"""CPU: the float64 yardstick of Synaptic Intelligence (tests/si_ref.py), the conditions of the GPU Trainer case along the oracle's
trajectory, and the plugin's place in the package."""
import types

import numpy as np
import pytest
import torch

from mafed_amd import SI
from tests.si_ref import SI_TRAINER, make_torch_si, si_accumulate_fp64, si_consolidate_fp64, si_stash_fp64, si_trainer_fp64


def _state(seed, n=4097):
    rng = np.random.default_rng(seed)
    g, p, anchor = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    return g, p, np.abs(rng.standard_normal(n)), anchor


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_penalty_gradient_is_the_gradient_of_the_penalty(seed):
    """g' - g of the statement against autograd of c sum Omega (p - p*)^2 in float64, and the penalty value itself."""
    g, p, omega, anchor = _state(seed)
    c = 0.75
    gp, term, s = si_stash_fp64(g, p, omega, anchor, 2 * c)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    pen = c * (torch.tensor(omega) * (pt - torch.tensor(anchor)) ** 2).sum()
    pen.backward()
    np.testing.assert_allclose(term, pt.grad.numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(gp - g, term, rtol=0, atol=1e-15 * np.abs(g).max() + 1e-15 * np.abs(term).max())
    assert abs(c * s - float(pen.detach())) <= 1e-13 * float(pen.detach())
    # task 0: g itself, no penalty
    g0, t0, s0 = si_stash_fp64(g, p)
    assert g0.tobytes() == np.asarray(g, np.float64).tobytes() and not t0.any() and s0 == 0.0


def test_consolidation_algebra():
    g, p, omega, anchor = _state(5)
    w = np.random.default_rng(6).standard_normal(p.size)
    xi = SI().xi                      # the plugin's default: 1e-3
    w[:64] = -1e6                      # a strongly negative path integral: the clamp gives exactly 0
    om, q = si_consolidate_fp64(omega, w, p, anchor, xi)
    assert (om[:64] == 0.0).all() and not np.signbit(om[:64]).any() and (om >= 0).all()
    keep = omega + q > 0
    np.testing.assert_array_equal(om[keep], (omega + w / ((p - anchor) ** 2 + xi))[keep])
    # the twin plugin states the same three assignments: Omega as above, p* == p and w == 0 afterwards
    TorchSI = make_torch_si()
    si = TorchSI(reg_lambda=1.0, xi=xi)
    model = types.SimpleNamespace(flat_params=torch.tensor(p, dtype=torch.float32))
    si.small_omega, si.omega, si.anchor = (torch.tensor(x, dtype=torch.float32) for x in (w, omega, anchor))
    want, _ = si_consolidate_fp64(si.omega.numpy(), si.small_omega.numpy(), model.flat_params.numpy(), si.anchor.numpy(), xi)
    si.update(model)
    assert si.task_id == 1 and torch.equal(si.anchor, model.flat_params) and not si.small_omega.any()
    np.testing.assert_allclose(si.omega.double().numpy(), want, rtol=2.0 ** -23, atol=0)
    assert (si.omega[:64] == 0).all()


def test_unmoved_elements_contribute_exactly_nothing():
    g, p, _, _ = _state(7)
    w = np.random.default_rng(8).standard_normal(p.size)
    sp = p.copy()
    sp[::2] += 1e-3
    sg = g.copy()
    sg[1::4] = np.inf
    sg[3::4] = np.nan                  # odd indices did not move: a non-finite g^ there leaves no trace
    w2, inc = si_accumulate_fp64(w, sg, sp, p)
    assert w2[1::2].tobytes() == w[1::2].tobytes() and not inc[1::2].any()
    np.testing.assert_array_equal(w2[::2], w[::2] - sg[::2] * (p[::2] - sp[::2]))


def test_path_integral_equals_the_loss_decrease():
    """Plain SGD with a small step on a quadratic L = 1/2 p'Ap - b'p: sum w = L(p_0) - L(p_T) to second order in the step.  Per step
    -g.dp = L(p) - L(p + dp) + 1/2 dp'A dp, and the second-order remainders sum to about eta / 2 times the decrease."""
    rng = np.random.default_rng(11)
    n, eta, T = 64, 1e-3, 200
    M = rng.standard_normal((n, n))
    A, b = M @ M.T / n + np.eye(n), rng.standard_normal(n)
    L = lambda x: 0.5 * x @ A @ x - b @ x
    p = rng.standard_normal(n)
    p0, w = p.copy(), np.zeros(n)
    for _ in range(T):
        g, sp = A @ p - b, p.copy()
        p = p - eta * g
        w, _ = si_accumulate_fp64(w, g, sp, p)
    drop = L(p0) - L(p)
    lam_max = float(np.linalg.eigvalsh(A).max())
    assert drop > 0 and (w >= 0).all()   # every SGD step moves each coordinate against its own gradient
    assert abs(w.sum() - drop) <= 0.5 * eta * lam_max * w.sum() * (1 + 1e-9)
    assert abs(w.sum() - drop) >= 1e-6 * drop, "the case cannot tell first order from exact"


def test_trainer_case_conditions():
    """tests/test_gpu_si.py::test_si_trainer_matches_torch_double along the float64 trajectory, c = 256, xi = 1e-3: the penalty gradient
    is zero on steps 0 .. 2 (task 0, then p == p* right behind the update) and on step 3 has norm 2.0859 against a task gradient of
    3.7864: ratio 0.551, inside [0.1, 10]; penalty 0.28343.  91.8 % of the parameters have Omega > 0 (at least 10 % asked).  Against
    the same run with c = 0 the final parameters differ by 4.9e-4, above 100 x the GPU test's parameter bound of 1e-6."""
    k = SI_TRAINER
    assert k["xi"] == 1e-3 and k["accumulate"] == 2 and k["update_after"] == 4 and k["n_micro"] == 8
    ref = si_trainer_fp64()
    for i, s in enumerate(ref["steps"]):
        print("[si] trainer step %d: |g| %.6g, |2c Omega (p - p*)| %.6g, penalty %.6g" % (i, s["g_norm"], s["term_norm"], s["penalty"]))
    print("[si] Omega > 0 on %.4f of the parameters" % ref["omega_pos"])
    assert [s["term_norm"] for s in ref["steps"][:3]] == [0.0, 0.0, 0.0]
    last = ref["steps"][3]
    ratio = last["term_norm"] / last["g_norm"]
    assert 0.1 <= ratio <= 10.0
    assert abs(ratio - 0.551) <= 1e-3 and abs(last["term_norm"] - 2.0859) <= 1e-3 and abs(last["penalty"] - 0.28343) <= 1e-4
    assert ref["omega_pos"] >= 0.10 and abs(ref["omega_pos"] - 0.918) <= 1e-3
    d = float((ref["params"] - si_trainer_fp64(0.0)["params"]).abs().max())
    print("[si] c = %g against c = 0: parameters differ by %.3e" % (k["c"], d))
    assert d > 100 * 1e-6 and abs(d - 4.9e-4) <= 1e-5


def test_si_is_exported_and_not_registered():
    import mafed_amd
    from mafed_amd import CLMethod
    from mafed_amd.methods import SI as SI2, CLStrategy, LwF
    assert SI is SI2 and mafed_amd.methods.si.SI is SI and issubclass(SI, CLStrategy)
    assert "si" not in CLMethod and "agem" not in CLMethod and CLMethod.extensions == {"lwf": LwF}
    assert set(CLMethod) == {"naive", "ewc", "replay", "featdistill"}
    si = SI()
    assert si.reg_lambda == 1.0 and si.xi == 1e-3 and si.task_id == 0
    assert si.grads_only_through_model is False and si.single_process_only is True
    assert si.small_omega is None and si.omega is None and si.anchor is None and si.last_penalty is None
    assert si.compute_loss(None, 1.5) == 1.5
    assert si.replay(None) == (None, 0)
    assert si.state_dict() == {"omega": None, "anchor": None, "small_omega": None, "task_id": 0}
    si2 = SI(reg_lambda=3.0, xi=0.1, opts=types.SimpleNamespace(accumulate_grad_batches=2))
    assert si2.reg_lambda == 3.0 and si2.xi == 0.1 and si2.update_freq == 2
    with pytest.raises(ValueError):
        SI(xi=0.0)
    foreign = torch.nn.Linear(2, 2)
    for call in (lambda: si.update(foreign), lambda: si.update_after_backward(model=foreign), lambda: si.update_after_step(model=foreign, batch_idx=0)):
        with pytest.raises(TypeError, match="native model"):
            call()
    assert si.task_id == 0


def test_si_state_dict_round_trip():
    a = SI(reg_lambda=2.0)
    a.omega, a.anchor, a.small_omega, a.task_id = torch.arange(8.0), torch.ones(8), -torch.arange(8.0), 2
    sd = a.state_dict()
    assert set(sd) == {"omega", "anchor", "small_omega", "task_id"}
    b = SI()
    b.load_state_dict(sd)
    assert b.task_id == 2 and all(torch.equal(getattr(a, k), getattr(b, k)) and getattr(a, k) is not getattr(b, k) for k in ("omega", "anchor", "small_omega"))
    with pytest.raises(ValueError):
        b.load_state_dict({"omega": sd["omega"]})


def test_trainer_refuses_a_reducer_for_si():
    """The guard sits in front of everything that needs a GPU: a stub model is enough."""
    from mafed_amd import Trainer
    with pytest.raises(ValueError, match="single-process"):
        Trainer(types.SimpleNamespace(), SI(), reducer=object())
    with pytest.raises(ValueError, match="single-process"):
        Trainer(types.SimpleNamespace(), SI(), ddp=True)
