"""CPU: the float64 restatement of MAS (tests/mas_ref.py) against autograd and against its own algebra, and the conditions of the
Trainer case that tests/test_gpu_mas.py runs on the GPU."""
import numpy as np
import torch

from tests.mas_ref import (MAS_TRAINER, mas_accumulate_fp64, mas_consolidate_fp64, mas_importances_fp64, mas_loader, mas_objective,
                           mas_penalty_fp64, mas_trainer_fp64, sqnorm_fp64)


def _head_case(B=3, T=5, V=8, seed=5):
    """Logits and labels with a sample without a labelled row (1), a label in the last position (sample 0: the shift hands it to row T - 2;
    the last row itself is never labelled) and a label in position 0 (sample 2: the shift drops it)."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(B, T, V, generator=gen, dtype=torch.float64)
    lab = torch.full((B, T), -100, dtype=torch.int64)
    lab[0, 2], lab[0, T - 1] = 3, 1
    lab[2, 0:4] = torch.tensor([5, 0, V - 1, 2])
    return z, lab


def test_objective_and_gradient_match_autograd():
    z, lab = _head_case()
    zt = z.clone().requires_grad_(True)
    J = mas_objective(zt, lab)
    (0.75 * J).backward()
    rowsq, J64, dz = sqnorm_fp64(z.numpy(), lab.numpy(), dloss=0.75)
    assert abs(float(J.detach()) - J64) <= 1e-14 * abs(J64)
    assert np.allclose(zt.grad.numpy(), dz, rtol=1e-14, atol=0.0)
    # rows: sample 0 has rows 1 and T - 2 (the label in the last position labels row T - 2), sample 1 none, sample 2 rows 0 .. 2
    m = rowsq != 0
    assert m.tolist() == [[False, True, False, True, False], [False] * 5, [True, True, True, False, False]]
    assert not dz[1].any() and not dz[:, -1].any()
    # by hand: J = (sum of sample 0's two rows / 2 + 0 / 1e-13 + sum of sample 2's three rows / 3) / 3
    z2 = (z.numpy() ** 2).sum(-1)
    assert abs(J64 - ((z2[0, 1] + z2[0, 3]) / 2 + z2[2, :3].sum() / 3) / 3) <= 1e-14 * J64


def test_objective_ignores_label_values():
    z, lab = _head_case()
    other = torch.where(lab != -100, (lab + 3) % 8, lab)
    assert float(mas_objective(z, lab)) == float(mas_objective(z, other))
    assert np.array_equal(sqnorm_fp64(z.numpy(), lab.numpy())[2], sqnorm_fp64(z.numpy(), other.numpy())[2])


def test_penalty_gradient_matches_autograd():
    gen = torch.Generator().manual_seed(11)
    n, c = 257, 1.75
    g, p, anchor = (torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(3))
    omega = torch.randn(n, generator=gen, dtype=torch.float64).abs()
    pt = p.clone().requires_grad_(True)
    pen = c * (omega * (pt - anchor) ** 2).sum()
    pen.backward()
    got, term, s = mas_penalty_fp64(g.numpy(), p.numpy(), omega.numpy(), anchor.numpy(), 2.0 * c)
    assert np.allclose(term, pt.grad.numpy(), rtol=1e-14, atol=0.0)
    assert np.allclose(got, (g + pt.grad).numpy(), rtol=1e-14, atol=1e-15)
    assert abs(c * s - float(pen.detach())) <= 1e-13 * float(pen.detach())


def test_consolidation_algebra():
    rng = np.random.default_rng(3)
    n, N, alpha = 64, 5, 0.25
    acc1, acc2 = rng.random(n) * 7, rng.random(n) * 7
    om1, old, new = mas_consolidate_fp64(None, acc1, N, alpha, first=True)
    assert np.array_equal(om1, acc1 / N) and not old.any() and np.array_equal(new, om1)
    om2, old, new = mas_consolidate_fp64(om1, acc2, N, alpha, first=False)
    assert np.allclose(om2, alpha * acc1 / N + (1 - alpha) * acc2 / N, rtol=1e-15) and np.array_equal(om2, old + new)
    # alpha = 1 keeps the old importance, alpha = 0 replaces it; equal importances are a fixed point for every alpha
    assert np.array_equal(mas_consolidate_fp64(om1, acc2, N, 1.0, False)[0], om1)
    assert np.array_equal(mas_consolidate_fp64(om1, acc2, N, 0.0, False)[0], acc2 / N)
    assert np.allclose(mas_consolidate_fp64(om1, acc1, N, alpha, False)[0], om1, rtol=1e-15)


def test_importance_is_even_in_the_gradient():
    rng = np.random.default_rng(4)
    g, acc = rng.standard_normal(100), rng.random(100)
    g[7] = -0.0
    a, inc = mas_accumulate_fp64(acc, g, 3.0)
    b, _ = mas_accumulate_fp64(acc, -g, 3.0)
    assert np.array_equal(a, b) and bool((inc >= 0).all()) and not np.signbit(inc[7])
    assert np.array_equal(a, acc + 3.0 * np.abs(g))


def test_importance_pass_weighs_batches_by_size():
    """Two batches of sizes 3 and 2: Omega = (3 |grad J(batch 0)| + 2 |grad J(batch 1)|) / 5, not the mean of the two."""
    from tests.helpers import trainer_case
    cfg, sd, _, batches = trainer_case()
    loader = mas_loader(batches)
    assert [b["input_ids"].shape[0] for b in loader] == [3, 2]
    both = mas_importances_fp64(cfg, sd, loader)
    one = [mas_importances_fp64(cfg, sd, [b]) for b in loader]
    for k in both:
        assert torch.allclose(both[k], (3 * one[0][k] + 2 * one[1][k]) / 5, rtol=1e-12, atol=0.0), k
    assert float(both["embed_out.weight"].abs().max()) > 0 and bool((both["embed_out.weight"] >= 0).all())


def test_trainer_case_conditions():
    """What tests/test_gpu_mas.py::test_mas_trainer_matches_torch_double relies on: no penalty on task 0 and on the first step of task 1
    (p = p*), a penalty gradient of the order of the task gradient on the last step, most parameters with Omega > 0, and a run that
    c = 0 would not reproduce."""
    k = MAS_TRAINER
    r, z = mas_trainer_fp64(), mas_trainer_fp64(0.0)
    s = r["steps"]
    print("[mas] fp64 trajectory:", [(round(x["g_norm"], 4), round(x["term_norm"], 4), round(x["penalty"], 5)) for x in s], "omega > 0:", r["omega_pos"])
    assert len(s) == k["n_micro"] // k["accumulate"]
    assert all(x["term_norm"] == 0.0 and x["penalty"] == 0.0 for x in s[:k["update_after"] + 1])
    assert 0.2 <= s[-1]["term_norm"] / s[-1]["g_norm"] <= 2.0 and s[-1]["penalty"] > 0
    assert r["omega_pos"] >= 0.5
    assert float((r["params"] - z["params"]).abs().max()) > 100 * 1e-6
