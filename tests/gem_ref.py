"""float64 restatement of GEM's projection and the oracle cases the GPU tests run (test infrastructure).

    gram[a][b] = sum x_a x_b (x_0 = g, x_k = r_k)    q_k = gram[0][k]    P = gram[1..K][1..K] + eps I
    every q_k >= 0: v = 0.    Else v = argmin 1/2 v'Pv + q'v s.t. v_k >= margin    g~ = g + sum_k v_k r_k
    (u = v - margin >= 0, q' = q + margin P 1; the supports S of u are enumerated and each P_SS u_S = -q'_S is solved by Cholesky)
"""
import numpy as np
import torch

from oracle import vlpythia_ref as R
from tests.helpers import golden_setup, step_fp64

GEM_MAX_REFS = 8
PIVOT_TOL, U_TOL, W_TOL = 1e-12, 1e-9, 1e-9


def gem_gram(g, refs):
    """(gram, sabs): the (K + 1) x (K + 1) matrix of inner products of x_0 = g, x_k = refs[k - 1] in float64, and sum |x_a x_b| beside it."""
    X = np.stack([np.asarray(x, np.float64).reshape(-1) for x in [g] + list(refs)])
    return X @ X.T, np.abs(X) @ np.abs(X).T


def qp_of(gram, margin, eps):
    """(P, q, q') of a Gram matrix."""
    gram = np.asarray(gram, np.float64)
    K = gram.shape[0] - 1
    P = gram[1:, 1:] + eps * np.eye(K)
    q = gram[0, 1:].copy()
    return P, q, q + margin * P.sum(axis=1)


def _cholesky_solve(A, b, thr):
    """x with A x = b by Cholesky (row by row, in float64), or None if a pivot is <= thr."""
    n = len(b)
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > thr:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def enumerate_supports(P, qp):
    """[(mask, u, w, objective, feasible, margins)] for every support whose Cholesky goes through; ``margins`` = (min u_S + tol, min
    w_offS + tol) -- how far the two feasibility tests are from flipping (inf where a test has nothing to look at)."""
    K = len(qp)
    thr = PIVOT_TOL * P.diagonal().max()
    maxq = np.abs(qp).max()
    out = []
    for mask in range(1 << K):
        S = [k for k in range(K) if mask >> k & 1]
        off = [k for k in range(K) if not mask >> k & 1]
        u = np.zeros(K)
        if S:
            us = _cholesky_solve(P[np.ix_(S, S)], -qp[S], thr)
            if us is None:
                continue
            u[S] = us
        w = P @ u + qp
        obj = float(np.sum(u * (0.5 * (w - qp) + qp)))
        mu = (u[S].min() + U_TOL * np.abs(u[S]).max()) if S else np.inf
        mw = (w[off].min() + W_TOL * maxq) if off else np.inf
        out.append((mask, u, w, obj, bool(mu >= 0 and mw >= 0 and np.isfinite(obj)), (mu, mw)))
    return out


def gem_solve(gram, margin, eps):
    """The enumeration solve as specified -> {"v" (float64, before any rounding), "u", "violated", "mask", "support" (its size), "P", "q", "qp"}.
    Lowest objective among the feasible supports, the lowest mask on a tie; a non-finite Gram or no feasible support: v = NaN."""
    gram = np.asarray(gram, np.float64)
    K = gram.shape[0] - 1
    assert 1 <= K <= GEM_MAX_REFS
    P, q, qp = qp_of(gram, margin, eps)
    res = {"P": P, "q": q, "qp": qp, "mask": 0, "support": 0, "u": np.zeros(K)}
    if not np.isfinite(gram).all():
        return dict(res, v=np.full(K, np.nan), violated=True)
    if (q >= 0).all():
        return dict(res, v=np.zeros(K), violated=False)
    best = None
    for mask, u, w, obj, ok, _ in enumerate_supports(P, qp):
        if ok and (best is None or obj < best[3]):
            best = (mask, u, w, obj)
    if best is None:
        return dict(res, v=np.full(K, np.nan), violated=True)
    u = np.maximum(best[1], 0.0)
    return dict(res, v=u + margin, u=u, violated=True, mask=best[0], support=bin(best[0]).count("1"))


def decision_gap(gram, margin, eps):
    """How clearly the enumeration decides, relative: the smallest distance of the chosen support's strictly complementary quantities
    from zero -- min over S of u_k / max|u| and min off S of w_k / max|q'| (inf where there is nothing to look at).  A problem with a
    gap far above the feasibility tolerances has one feasible support, and rounding cannot move the choice."""
    s = gem_solve(gram, margin, eps)
    P, qp, u = s["P"], s["qp"], s["u"]
    w = P @ u + qp
    S = [k for k in range(len(qp)) if s["mask"] >> k & 1]
    off = [k for k in range(len(qp)) if not s["mask"] >> k & 1]
    gu = (u[S].min() / np.abs(u[S]).max()) if S else np.inf
    gw = (w[off].min() / np.abs(qp).max()) if off else np.inf
    return float(min(gu, gw))


def kkt_residuals(P, qp, u):
    """Independent of how u was found: (primal, dual, complementarity) of min 1/2 u'Pu + q''u s.t. u >= 0, each relative --
    max(0, -u_k) / max|u|, max(0, -w_k) / s_k and |u_k w_k| / (max|u| s_k) with w = P u + q' and s_k = sum_j |P_kj| |u_j| + |q'_k|, the
    size of the terms w_k is the sum of."""
    P, qp, u = (np.asarray(x, np.float64) for x in (P, qp, u))
    w = P @ u + qp
    s = np.abs(P) @ np.abs(u) + np.abs(qp)
    s = np.where(s > 0, s, 1.0)
    umax = np.abs(u).max() or 1.0
    return float(np.maximum(-u, 0).max() / umax), float((np.maximum(-w, 0) / s).max()), float((np.abs(u * w) / (umax * s)).max())


def pgd_solve(P, qp, iters=200000, tol=1e-13):
    """min 1/2 u'Pu + q''u s.t. u >= 0 by accelerated projected gradient (step 1 / lambda_max, restart when the objective would rise), in
    float64: shares nothing with the enumeration.  Stops when an iteration moves u by less than tol max|u|."""
    P, qp = np.asarray(P, np.float64), np.asarray(qp, np.float64)
    step = 1.0 / np.linalg.eigvalsh(P)[-1]
    u = np.zeros(len(qp))
    y, t = u.copy(), 1.0
    for _ in range(iters):
        un = np.maximum(y - step * (P @ y + qp), 0.0)
        if np.dot(P @ y + qp, un - u) > 0:   # gradient restart
            y, t = u.copy(), 1.0
            un = np.maximum(y - step * (P @ y + qp), 0.0)
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        y = un + (t - 1.0) / tn * (un - u)
        moved = np.abs(un - u).max()
        u, t = un, tn
        if moved <= tol * max(np.abs(u).max(), 1e-300):
            break
    return u


def gem_project(g, refs, v, violated):
    """g~ in float64 (``g`` itself, as an array, when nothing is violated)."""
    g64 = np.asarray(g, np.float64)
    if not violated:
        return g64
    return g64 + sum(float(vk) * np.asarray(r, np.float64) for vk, r in zip(v, refs))


def spd_problem(K, seed, cond=1e6, active=None, margin=0.0):
    """A Gram matrix [(K + 1), (K + 1)] whose P block has the log-spaced spectrum 1 .. 1 / cond in a random orthogonal basis, and whose q
    makes exactly the constraints ``active`` (default: a random non-empty subset) the support at this margin and eps = 0, with every
    complementary quantity well away from zero on its scale: u_S and w off S are chosen first, q' = w - P u and q = q' - margin P 1
    follow."""
    rng = np.random.default_rng(100000 * K + seed)
    Q, _ = np.linalg.qr(rng.standard_normal((K, K)))
    P = (Q * np.logspace(0, -np.log10(cond), K)) @ Q.T if K > 1 else np.ones((1, 1))
    P = 0.5 * (P + P.T)
    if active is None:
        active = [k for k in range(K) if rng.random() < 0.5] or [int(rng.integers(K))]
    active = list(active)
    u, w = np.zeros(K), np.zeros(K)
    for k in range(K):
        if k in active:
            u[k] = rng.uniform(0.2, 2.0)
        else:
            w[k] = rng.uniform(0.2, 2.0)
    q = w * (np.abs(P @ u).max() or 1.0) - P @ u - margin * P.sum(axis=1)   # w off S on the scale of P u
    gram = np.zeros((K + 1, K + 1))
    gram[1:, 1:] = P
    gram[0, 1:] = gram[1:, 0] = q
    gram[0, 0] = 1.0 + float(q @ np.linalg.solve(P, q))   # (keeps the whole matrix positive definite; the solve does not read it)
    return gram, sorted(active)


def solve_suite():
    """The problems of the solve tests, [(K, seed, margin, gram, active)]: K = 2 .. 8 x 11 seeds at condition number 1e6, eps = 0.  Seed 0
    has every constraint in the support, seeds 1 .. 9 a random support of size 1 + (seed - 1) % K, seed 10 the empty one (u = 0: every
    coefficient on the margin); the margin alternates between 0 and 0.5 (seed 10: 0.5)."""
    out = []
    for K in range(2, GEM_MAX_REFS + 1):
        for seed in range(11):
            size = K if seed == 0 else (0 if seed == 10 else 1 + (seed - 1) % K)
            rng = np.random.default_rng(7000 + 100 * K + seed)
            active = sorted(int(k) for k in rng.choice(K, size=size, replace=False))
            margin = 0.5 if seed == 10 or (seed + K) % 2 else 0.0
            for j in range(100):   # (with a margin, q = q' - margin P 1 need not have a negative entry: the first draw that has one)
                gram = spd_problem(K, seed + 1000 * j, active=active, margin=margin)[0]
                if (gram[0, 1:] < 0).any():
                    break
            out.append((K, seed, margin, gram, active))
    return out


# ---- whole-step oracle cases ---------------------------------------------------------------------------------------------------
# (golden configuration, (memory seed of task 0, memory seed of task 1), margin) -> (violated, support size) expected from the float64
# oracle, eps = 1e-3.  Picked on the CPU from the memory seeds 900 .. 915: q_k / sum|g r_k| = -0.138 (902), -0.114 (907), +0.090 (905),
# +0.202 (915), and every chosen support is clear of its neighbours (decision_gap >= 0.8; tests/test_gem_ref.py).  The last case runs
# the default margin: q' = q + margin P 1 is positive there, so u = 0 and both coefficients sit on the margin.
ORACLE_CASES = {("t64", (905, 915), 0.0): (False, 0), ("t64", (902, 915), 0.0): (True, 1), ("t64", (902, 907), 0.0): (True, 2),
                ("t64", (902, 907), 0.5): (True, 0)}


def memory_batch(name, seed):
    """The memory batch of an oracle case: at the golden batch's B, T."""
    cfg, _, _, batch, _ = golden_setup(name)
    B, T = batch["input_ids"].shape
    return R.make_batch(cfg, B, T, seed=seed, pad=True, n_answer=3)


_GRADS, _CASES = {}, {}


def _grads(name, seed):
    key = (name, seed)
    if key not in _GRADS:
        cfg, sd, _, batch, _ = golden_setup(name)
        _GRADS[key] = step_fp64(cfg, sd, batch if seed is None else memory_batch(name, seed))["grads"]
    return _GRADS[key]


def oracle_case(name, seeds, margin, eps=1e-3):
    """{"g", "refs": float64 gradients {parameter: tensor} of the golden batch / of each memory batch at the golden weights, "names", "gram",
    "sabs", "solve": gem_solve of the Gram over all parameters}; computed once and shared (read only)."""
    key = (name, tuple(seeds), margin, eps)
    if key not in _CASES:
        cfg = golden_setup(name)[0]
        names = [k for k, _ in R.param_shapes(cfg)]
        g, refs = _grads(name, None), [_grads(name, s) for s in seeds]
        flat = lambda d: torch.cat([d[k].reshape(-1) for k in names]).numpy()
        gram, sabs = gem_gram(flat(g), [flat(r) for r in refs])
        _CASES[key] = {"g": g, "refs": refs, "names": names, "gram": gram, "sabs": sabs, "solve": gem_solve(gram, margin, eps)}
    return _CASES[key]


# The Trainer case of tests/test_gpu_gem.py: micro-batches 0 .. 7 of tests.helpers.trainer_case() (task-batch seeds 33 .. 40) at
# accumulate = 2, two finished tasks whose memories hold exactly its memory batches ``memories`` (one each), task 2, no warm-up and a
# linear decay over 100 steps as in tests/agem_ref.py.
GEM_TRAINER = dict(n_micro=8, memories=(1, 4), margin=0.0, eps=1e-3, accumulate=2, lr=1e-3, betas=(0.9, 0.98), adam_eps=1e-6,
                   weight_decay=0.01, grad_clip=2.0, warmup=0, total_steps=100)
# What gem_trainer_fp64() gives per optimiser step, (violated, support mask), checked by tests/test_gem_ref.py.  Chosen among the pairs
# of memory batches 0 .. 5 so that the windows' (q_1, q_2) / sum|g r_k| go (+0.133, -0.094), (-0.195, -0.132), (-0.200, -0.035),
# (+0.263, +0.151): task 1 alone, both, both, none -- each decision at least 0.18 of its scale away from flipping.
GEM_TRAINER_PATTERN = [(True, 0b10), (True, 0b11), (True, 0b11), (False, 0)]


def gem_trainer_fp64(case=None):
    """GEM_TRAINER in float64 with the oracle's forward, clip and AdamW (the window end of oracle RefTrainer.step with the projection in
    front of the clip): [{"gram", "sabs", "solve", "grad_norm"}] per optimiser step."""
    from tests.helpers import trainer_case
    c = case or GEM_TRAINER
    cfg, sd, _, batches = trainer_case()
    f64 = lambda b: dict(b, patch_embeddings=b["patch_embeddings"].double())
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    m, v = ({k: torch.zeros_like(p.detach()) for k, p in params.items()} for _ in range(2))
    names = list(params)
    mems = [f64(batches[i][1]) for i in c["memories"]]
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).numpy()
    out = []
    for i in range(c["n_micro"]):
        (R.forward(params, f64(batches[i][0]), cfg).loss / c["accumulate"]).backward()
        if (i + 1) % c["accumulate"]:
            continue
        step = len(out) + 1
        refs = []
        for mem in mems:
            r = torch.autograd.grad(R.forward(params, mem, cfg).loss, [params[k] for k in names], allow_unused=True)
            refs.append([torch.zeros_like(params[k].detach()) if x is None else x for k, x in zip(names, r)])
        g = [params[k].grad for k in names]
        gram, sabs = gem_gram(flat(g), [flat(r) for r in refs])
        sol = gem_solve(gram, c["margin"], c["eps"])
        if sol["violated"]:
            g = [a + sum(float(vk) * r[j] for vk, r in zip(sol["v"], refs)) for j, a in enumerate(g)]
        norm, scale = R.clip_grad_norm(g, c["grad_clip"])
        out.append({"gram": gram, "sabs": sabs, "solve": sol, "grad_norm": float(norm)})
        lr = c["lr"] * R.lr_lambda(step - 1, c["warmup"], c["total_steps"])
        with torch.no_grad():
            for k, gk in zip(names, g):
                wd = c["weight_decay"] if R.param_group_of(k) % 2 == 0 else 0.0
                R.adamw_step(params[k], gk * scale, m[k], v[k], step, lr, c["betas"][0], c["betas"][1], c["adam_eps"], wd)
                params[k].grad = None
    return out
