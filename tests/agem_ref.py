"""float64 restatement of the A-GEM projection and the oracle cases the GPU tests run (test infrastructure).

    dot = sum g r    rsq = sum r r    alpha = dot / rsq if dot < 0 and rsq > 0, else 0    g' = g - alpha r   (alpha = 0: g' is g)
"""
import numpy as np
import torch

from oracle import vlpythia_ref as R
from tests.helpers import golden_setup, step_fp64


def agem_stats(g, r):
    """(dot, rsq, alpha, violated, sum |g r|) of two float64 vectors."""
    g, r = np.asarray(g, np.float64).reshape(-1), np.asarray(r, np.float64).reshape(-1)
    dot, rsq = float(np.dot(g, r)), float(np.dot(r, r))
    violated = dot < 0.0 and rsq > 0.0
    return dot, rsq, (dot / rsq if violated else 0.0), violated, float(np.abs(g * r).sum())


def agem_project(g, r):
    """g' (float64; ``g`` itself, as an array, when nothing is violated) and agem_stats(g, r)."""
    st = agem_stats(g, r)
    g64, r64 = np.asarray(g, np.float64), np.asarray(r, np.float64)
    return (g64 - st[2] * r64 if st[3] else g64), st


# (golden configuration, memory seed or "self" = the golden batch itself) -> expected sign of dot (-1: violated)
ORACLE_CASES = {("t64", 902): -1, ("t128", 901): -1, ("t128", 903): +1, ("t64", "self"): +1}


def memory_batch(name, seed):
    """The memory batch of an oracle case: at the golden batch's B, T."""
    cfg, _, _, batch, _ = golden_setup(name)
    if seed == "self":
        return {k: v.clone() for k, v in batch.items()}
    B, T = batch["input_ids"].shape
    return R.make_batch(cfg, B, T, seed=seed, pad=True, n_answer=3)


_CASES = {}


def oracle_case(name, seed):
    """{"g", "r": {parameter: float64 gradient} of the golden batch / the memory batch at the golden weights, "stats": agem_stats over all
    parameters, "names"}; computed once and shared (read only)."""
    key = (name, seed)
    if key not in _CASES:
        cfg, sd, _, batch, _ = golden_setup(name)
        g = step_fp64(cfg, sd, batch)["grads"]
        r = g if seed == "self" else step_fp64(cfg, sd, memory_batch(name, seed))["grads"]
        names = [k for k, _ in R.param_shapes(cfg)]
        flat = lambda d: torch.cat([d[k].reshape(-1) for k in names]).numpy()
        _CASES[key] = {"g": g, "r": r, "names": names, "stats": agem_stats(flat(g), flat(r))}
    return _CASES[key]


# The Trainer case of tests/test_gpu_agem.py: micro-batches 0 .. 7 of tests.helpers.trainer_case() (task-batch seeds 33 .. 40) at
# accumulate = 2, the memory holding exactly memory batch 1 (seed 74), task 1, no warm-up and a linear decay over 100 steps
# as in tests/test_gpu_lwf.py.  Chosen so that the windows' dots against that memory batch go +, -, -, +.
AGEM_TRAINER = dict(n_micro=8, memory=1, accumulate=2, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01, grad_clip=2.0,
                    warmup=0, total_steps=100)


def agem_trainer_fp64():
    """AGEM_TRAINER in float64 with the oracle's forward, clip and AdamW (the window end of oracle RefTrainer.step with the projection in
    front of the clip): [(dot, rsq, alpha, violated, sum|g r|)] per optimiser step."""
    from tests.helpers import trainer_case
    c = AGEM_TRAINER
    cfg, sd, _, batches = trainer_case()
    f64 = lambda b: dict(b, patch_embeddings=b["patch_embeddings"].double())
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    m, v = ({k: torch.zeros_like(p.detach()) for k, p in params.items()} for _ in range(2))
    names = list(params)
    mem = f64(batches[c["memory"]][1])
    out = []
    for i in range(c["n_micro"]):
        (R.forward(params, f64(batches[i][0]), cfg).loss / c["accumulate"]).backward()
        if (i + 1) % c["accumulate"]:
            continue
        step = len(out) + 1
        r = torch.autograd.grad(R.forward(params, mem, cfg).loss, [params[k] for k in names], allow_unused=True)
        r = [torch.zeros_like(params[k].detach()) if x is None else x for k, x in zip(names, r)]
        g = [params[k].grad for k in names]
        flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).numpy()
        st = agem_stats(flat(g), flat(r))
        out.append(st)
        g = [a - st[2] * b for a, b in zip(g, r)]
        _, scale = R.clip_grad_norm(g, c["grad_clip"])
        lr = c["lr"] * R.lr_lambda(step - 1, c["warmup"], c["total_steps"])
        with torch.no_grad():
            for k, gk in zip(names, g):
                wd = c["weight_decay"] if R.param_group_of(k) % 2 == 0 else 0.0
                R.adamw_step(params[k], gk * scale, m[k], v[k], step, lr, c["betas"][0], c["betas"][1], c["eps"], wd)
                params[k].grad = None
    return out
