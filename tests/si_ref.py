"""float64 restatement of Synaptic Intelligence's three passes, a twin plugin that runs them with torch ops, and the
Trainer case the GPU tests run (test infrastructure).

    pass A       g^ = g    p^ = p    from task 1 on  g' = g + 2c Omega (p - p*)      penalty = c sum Omega (p - p*)^2
    pass B       w' = w - g^ (p - p^)  where p != p^, else w
    consolidate  Omega' = max(Omega + w / ((p - p*)^2 + xi), 0)    p* = p    w = 0
"""
import numpy as np
import torch

from oracle import vlpythia_ref as R


def _f64(x):
    return np.asarray(x, np.float64)


def si_stash_fp64(g, p, omega=None, anchor=None, two_c=0.0):
    """(g', term, sum Omega (p - p*)^2) with term = 2c Omega (p - p*); without omega: (g, zeros, 0)."""
    g, p = _f64(g), _f64(p)
    if omega is None:
        return g, np.zeros_like(g), 0.0
    d = p - _f64(anchor)
    term = float(two_c) * _f64(omega) * d
    return g + term, term, float((_f64(omega) * d * d).sum())


def si_accumulate_fp64(w, stash_g, stash_p, p):
    """(w', g^ (p - p^) with 0 where the parameter did not move)."""
    w, sg, sp, p = _f64(w), _f64(stash_g), _f64(stash_p), _f64(p)
    moved = p != sp
    with np.errstate(invalid="ignore", over="ignore"):
        inc = np.where(moved, sg * (p - sp), 0.0)
    return np.where(moved, w - inc, w), inc


def si_consolidate_fp64(omega, w, p, anchor, xi):
    """(Omega', q = w / ((p - p*)^2 + xi))."""
    d = _f64(p) - _f64(anchor)
    q = _f64(w) / (d * d + float(xi))
    return np.maximum(_f64(omega) + q, 0.0), q


def make_torch_si():
    """``TorchSI``: the plugin's hooks with torch ops in float64 rounded to fp32, on whatever device the model lives.  No norm hand-over:
    the clip takes the one-pass norm.  For a Trainer without the pipelined optimiser."""
    from mafed_amd.methods.base import CLStrategy

    class TorchSI(CLStrategy):
        grads_only_through_model = False
        single_process_only = True

        def __init__(self, reg_lambda=1.0, xi=1e-3, **kwargs):
            super().__init__(reg_lambda, **kwargs)
            self.xi = float(xi)
            self.small_omega = self.omega = self.anchor = None
            self._pending = False
            self.last_penalty = None

        def compute_loss(self, model, loss, **kwargs):
            return loss

        def _ensure(self, model):
            if self.small_omega is None:
                p = model.flat_params
                self.small_omega, self.omega, self.anchor = torch.zeros_like(p), torch.zeros_like(p), p.detach().clone()

        def update(self, model, **kwargs):
            self._ensure(model)
            p = model.flat_params.double()
            d = p - self.anchor.double()
            self.omega = (self.omega.double() + self.small_omega.double() / (d * d + self.xi)).clamp_min(0.0).float()
            self.anchor = model.flat_params.detach().clone()
            self.small_omega = torch.zeros_like(self.small_omega)
            self.task_id += 1

        def update_after_backward(self, model=None, **kwargs):
            self._ensure(model)
            g, p = model.flat_grads, model.flat_params
            self._stash_g, self._stash_p = g.clone(), p.detach().clone()
            if self.task_id > 0:
                d = p.double() - self.anchor.double()
                g.copy_((g.double() + 2.0 * float(self.reg_lambda) * self.omega.double() * d).float())
                self.last_penalty = (float(self.reg_lambda) * (self.omega.double() * d * d).sum()).float()
            self._pending = True

        def update_after_step(self, model=None, **kwargs):
            if not self._pending:
                return
            self._pending = False
            p, sp = model.flat_params.double(), self._stash_p.double()
            w = self.small_omega.double()
            self.small_omega = torch.where(p != sp, w - self._stash_g.double() * (p - sp), w).float()

    return TorchSI


# The Trainer case of tests/test_gpu_si.py: micro-batches 0 .. 7 of tests.helpers.trainer_case() (task-batch seeds 33 .. 40) at
# accumulate = 2: two optimiser steps of task 0, update(model), two of task 1; no warm-up and a linear decay over 100 steps as in
# tests/agem_ref.py.  ``c`` is chosen on the CPU (tests/test_si_ref.py::test_trainer_case_conditions) so that the penalty gradient is
# of the order of the task gradient on the last step -- the first whose p - p* is not zero.
SI_TRAINER = dict(n_micro=8, accumulate=2, update_after=4, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01, grad_clip=2.0,
                  warmup=0, total_steps=100, xi=1e-3, c=256.0)

_TRAJ = {}


def si_trainer_fp64(c=None):
    """SI_TRAINER in float64 with the oracle's forward, clip and AdamW: {"steps": [{"g_norm", "term_norm", "penalty"}] per optimiser
    step, "omega_pos": fraction of parameters with Omega > 0 after the update, "params": the final flat parameters}.  Cached per c."""
    from tests.helpers import trainer_case
    k = SI_TRAINER
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
    w, omega, anchor, task = torch.zeros_like(theta()), torch.zeros_like(theta()), theta().clone(), 0
    steps, omega_pos = [], None
    for i in range(k["n_micro"]):
        if i == k["update_after"]:
            d = theta() - anchor
            omega = (omega + w / (d * d + k["xi"])).clamp_min(0.0)
            anchor, w, task = theta().clone(), torch.zeros_like(w), task + 1
            omega_pos = float((omega > 0).double().mean())
        (R.forward(params, f64(batches[i][0]), cfg).loss / k["accumulate"]).backward()
        if (i + 1) % k["accumulate"]:
            continue
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
        w = w - g_hat * (theta() - p_hat)
        steps.append(dict(g_norm=float(g_hat.norm()), term_norm=float(term.norm()), penalty=pen))
    _TRAJ[c] = dict(steps=steps, omega_pos=omega_pos, params=theta().clone())
    return _TRAJ[c]
