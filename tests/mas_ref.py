"""float64 restatement of Memory Aware Synapses: the squared-norm head objective, the three flat passes, the
importance pass under the oracle's autograd, a twin plugin that runs the hooks with torch ops, and the Trainer case the GPU tests run
(test infrastructure).

    objective    J = mean_b( sum_t |z[b,t]|^2 / max(count_b, 1e-13) ) over the rows whose shifted label is not -100
    accumulate   acc' = acc + w |g|
    consolidate  Omega' = acc / N (first task) or alpha Omega + (1 - alpha) acc / N    p* = p    acc = 0
    penalty      g' = g + 2c Omega (p - p*)      penalty = c sum Omega (p - p*)^2
"""
import numpy as np
import torch

from oracle import vlpythia_ref as R


def _f64(x):
    return np.asarray(x, np.float64)


# ---- the head objective ---------------------------------------------------------------------------------------------------------
def mas_objective(logits, labels):
    """J of text logits [B, T, V] (torch, differentiable) and labels [B, T]: the rows and the normaliser of R.masked_mean_loss, the
    label values unused."""
    z = logits[:, :-1, :]
    m = labels[:, 1:] != -100
    s = (z * z).sum(-1).masked_fill(~m, 0.0).sum(-1)
    return (s / m.sum(-1).to(s.dtype).clamp(min=1e-13)).mean()


def sqnorm_fp64(logits, labels, dloss=1.0):
    """Closed form in numpy float64: (rowsq [B, T], J, dJ/dz [B, T, V] times dloss); row (b, t) is labelled when t < T - 1 and
    labels[b, t + 1] != -100."""
    z, lab = _f64(logits), np.asarray(labels)
    B, T, _ = z.shape
    m = np.zeros((B, T), bool)
    m[:, :-1] = lab[:, 1:] != -100
    cnt = np.maximum(m.sum(1).astype(np.float64), 1e-13)
    rowsq = np.where(m, (z * z).sum(-1), 0.0)
    J = float((rowsq.sum(1) / cnt).mean())
    dz = np.where(m[:, :, None], 2.0 * float(dloss) * z / (B * cnt)[:, None, None], 0.0)
    return rowsq, J, dz


# ---- the flat passes ------------------------------------------------------------------------------------------------------------
def mas_accumulate_fp64(acc, g, w):
    """(acc + w |g|, w |g|)."""
    inc = float(w) * np.abs(_f64(g))
    return _f64(acc) + inc, inc


def mas_consolidate_fp64(omega, acc, seen, alpha, first):
    """(Omega', old term alpha Omega (zeros on the first task), new term (1 - alpha) acc / N (acc / N on the first task))."""
    new = _f64(acc) / float(seen)
    if first:
        return new, np.zeros_like(new), new
    old, new = float(alpha) * _f64(omega), (1.0 - float(alpha)) * new
    return old + new, old, new


def mas_penalty_fp64(g, p, omega, anchor, two_c):
    """(g', term = 2c Omega (p - p*), sum Omega (p - p*)^2)."""
    d = _f64(p) - _f64(anchor)
    term = float(two_c) * _f64(omega) * d
    return _f64(g) + term, term, float((_f64(omega) * d * d).sum())


# ---- the importance pass under the oracle's autograd ----------------------------------------------------------------------------
def mas_importances_fp64(cfg, sd, batches):
    """{name: Omega_new} = sum over batches of n |grad J| / N with the oracle's forward in float64 and J = mas_objective on its text
    logits.  A parameter J does not reach gets exact zeros."""
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    acc = {k: torch.zeros_like(v.detach()) for k, v in params.items()}
    seen = 0
    for b in batches:
        n, T = b["input_ids"].shape
        out = R.forward(params, dict(b, patch_embeddings=b["patch_embeddings"].double(), labels=None), cfg)
        grads = torch.autograd.grad(mas_objective(out.logits[:, -T:], b["labels"]), list(params.values()), allow_unused=True)
        for k, g in zip(params, grads):
            if g is not None:
                acc[k] += n * g.abs()
        seen += n
    return {k: v / seen for k, v in acc.items()}


# ---- the twin plugin ------------------------------------------------------------------------------------------------------------
def make_torch_mas():
    """``TorchMAS``: the plugin's hooks with torch ops in float64 rounded to fp32, on whatever device the model lives.  The importance
    pass runs the model's own forward and backward under ``head_loss = SquaredNorm()``; everything behind the gradient is torch.  No norm
    hand-over: the clip takes the one-pass norm."""
    from mafed_amd.methods.base import CLStrategy

    class TorchMAS(CLStrategy):
        grads_only_through_model = False
        single_process_only = True

        def __init__(self, reg_lambda=1.0, alpha=0.5, **kwargs):
            super().__init__(reg_lambda, **kwargs)
            self.alpha = float(alpha)
            self.omega = self.anchor = self.last_penalty = None

        def compute_loss(self, model, loss, **kwargs):
            return loss

        def update(self, model, dataloader=None, **kwargs):
            from mafed_amd.head_loss import SquaredNorm
            acc, seen = torch.zeros_like(model.flat_params, dtype=torch.float64), 0
            previous, model.head_loss = model.head_loss, SquaredNorm()
            try:
                for batch in dataloader:
                    model.zero_grad()
                    n = batch["input_ids"].size(0)
                    model(**batch, compute_loss=True, return_dict=True).loss.backward()
                    acc += n * model.flat_grads.double().abs()
                    seen += n
            finally:
                model.head_loss = previous
            model.zero_grad()
            new = acc / seen
            self.omega = (new if self.task_id == 0 else self.alpha * self.omega.double() + (1.0 - self.alpha) * new).float()
            self.anchor = model.flat_params.detach().clone()
            self.task_id += 1

        def update_after_backward(self, model=None, **kwargs):
            if self.task_id == 0:
                return
            g, p = model.flat_grads, model.flat_params
            d = p.double() - self.anchor.double()
            g.copy_((g.double() + 2.0 * float(self.reg_lambda) * self.omega.double() * d).float())
            self.last_penalty = (float(self.reg_lambda) * (self.omega.double() * d * d).sum()).float()

    return TorchMAS


# The Trainer case of tests/test_gpu_mas.py: micro-batches 0 .. 5 of tests.helpers.trainer_case() at accumulate = 1: three optimiser steps
# of task 0, update(model, loader), three of task 1; the importance loader is micro-batch 6 whole (3 samples) and the first 2 samples of
# micro-batch 7.  No warm-up and a linear decay over 100 steps as in tests/si_ref.py.  ``c`` is chosen on the CPU
# (tests/test_mas_ref.py::test_trainer_case_conditions) so that the penalty gradient is of the order of the task gradient on the last
# step; on the first step of task 1 it is zero (p = p*).
MAS_TRAINER = dict(n_micro=6, accumulate=1, update_after=3, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01, grad_clip=2.0,
                   warmup=0, total_steps=100, alpha=0.5, c=4.0)


def mas_loader(batches):
    """The importance loader of MAS_TRAINER from tests.helpers.trainer_case()'s micro-batches: sizes 3 and 2."""
    return [dict(batches[6][0]), {k: v[:2].clone() for k, v in batches[7][0].items()}]


_TRAJ = {}


def mas_trainer_fp64(c=None):
    """MAS_TRAINER in float64 with the oracle's forward, clip and AdamW: {"steps": [{"g_norm", "term_norm", "penalty"}] per optimiser
    step, "omega_pos": fraction of parameters with Omega > 0, "params": the final flat parameters}.  Cached per c."""
    from tests.helpers import trainer_case
    k = MAS_TRAINER
    c = float(k["c"] if c is None else c)
    if c in _TRAJ:
        return _TRAJ[c]
    cfg, sd, _, batches = trainer_case()
    f64 = lambda b: dict(b, patch_embeddings=b["patch_embeddings"].double())
    params = {n: v.double().clone().requires_grad_(True) for n, v in sd.items()}
    names = list(params)
    m, v = ({n: torch.zeros_like(p.detach()) for n, p in params.items()} for _ in range(2))
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])
    split = lambda t: [x.view_as(params[n]) for n, x in zip(names, t.split([params[n].numel() for n in names]))]
    theta = lambda: flat([params[n] for n in names])
    omega, anchor, task = torch.zeros_like(theta()), theta().clone(), 0
    steps, omega_pos = [], None
    for i in range(k["n_micro"]):
        if i == k["update_after"]:
            imp = mas_importances_fp64(cfg, {n: p.detach() for n, p in params.items()}, mas_loader(batches))
            omega, anchor, task = flat([imp[n] for n in names]), theta().clone(), task + 1
            omega_pos = float((omega > 0).double().mean())
        R.forward(params, f64(batches[i][0]), cfg).loss.backward()
        step = len(steps) + 1
        g_hat, p_hat = flat([params[n].grad for n in names]), theta().clone()
        term = 2.0 * c * omega * (p_hat - anchor) if task > 0 else torch.zeros_like(g_hat)
        pen = c * float((omega * (p_hat - anchor) ** 2).sum()) if task > 0 else 0.0
        g = split(g_hat + term)
        _, scale = R.clip_grad_norm(g, k["grad_clip"])
        lr = k["lr"] * R.lr_lambda(step - 1, k["warmup"], k["total_steps"])
        with torch.no_grad():
            for n, gn in zip(names, g):
                wd = k["weight_decay"] if R.param_group_of(n) % 2 == 0 else 0.0
                R.adamw_step(params[n], gn * scale, m[n], v[n], step, lr, k["betas"][0], k["betas"][1], k["eps"], wd)
                params[n].grad = None
        steps.append(dict(g_norm=float(g_hat.norm()), term_norm=float(term.norm()), penalty=pen))
    _TRAJ[c] = dict(steps=steps, omega_pos=omega_pos, params=theta().clone())
    return _TRAJ[c]
