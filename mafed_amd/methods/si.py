"""Synaptic Intelligence (Zenke, Poole, Ganguli 2017): the regulariser whose importance is collected online, inside the training step.

The reference ships no implementation, so the arithmetic is this project's.  The state is four flat fp32 buffers
laid out like ``model.flat_params``: the path integral w (``small_omega``), the importance Omega (``omega``), the anchor p* (``anchor``)
and the stash pair (g^, p^).  With c = ``reg_lambda``:

    pass A  update_after_backward, on the micro-batch that closes a window, in front of the clip
            g^ = g    p^ = p    from task 1 on  g += 2c Omega (p - p*)  in place; leaves the clip's sum-of-squares partials of the g it
            leaves (``model.final_grad_sumsq``) and ``last_penalty`` = c sum Omega (p - p*)^2
    pass B  update_after_step, behind the optimiser, when a pass A is pending
            w -= g^ (p - p^)  where p moved; an unmoved element keeps its w bit for bit (a skipped step leaves no trace)
    update  between tasks:  Omega = max(Omega + w / ((p - p*)^2 + xi), 0)    p* = p    w = 0    task_id += 1

g^ is the unregularised gradient, as in the paper; the clip scale, the weight decay and the optimiser rule are all inside p - p^.  The
penalty never enters autograd -- ``compute_loss`` returns the loss unchanged -- so its gradient is added once per window, after the last
backward, whatever the backward did to the gradient buffer before (overwriting weight-gradient sweeps included).  Nothing here
synchronises with the host.  The passes are ``csrc/si.hip``.
"""
from __future__ import annotations

from typing import Optional

import torch

from mafed_amd import ops
from mafed_amd.methods.base import CLStrategy
from mafed_amd.methods.flat import FlatPlugin, behind_optimizer


class SI(FlatPlugin, CLStrategy):
    """``SI(reg_lambda=1.0, xi=1e-3)``.  ``xi`` damps the division where a parameter barely moved; 1e-3 is the paper's CIFAR value and has
    not been tuned for this model."""
    _STATE = (("omega", torch.float32), ("anchor", torch.float32), ("small_omega", torch.float32))

    def __init__(self, reg_lambda=1.0, xi=1e-3, **kwargs):
        super().__init__(reg_lambda, **{k: v for k, v in kwargs.items() if k in ("mask", "scaler", "opts")})
        if not xi > 0:
            raise ValueError("xi must be positive")
        self.xi = float(xi)
        self.small_omega: Optional[torch.Tensor] = None   # w: the running path integral of the task being learnt
        self.omega: Optional[torch.Tensor] = None         # consolidated importance
        self.anchor: Optional[torch.Tensor] = None        # parameters at the last consolidation (task 0: at the first pass A)
        self._stash_g = self._stash_p = self._pen = None
        self.last_penalty: Optional[torch.Tensor] = None  # device scalar c sum Omega (p - p*)^2 of the last pass A; None until the first
        self._pending = False                             # a pass A whose pass B has not run yet

    # ---- buffers -----------------------------------------------------------------------------------------------------------
    def _ensure(self, model) -> None:
        """Allocate once: the state at the first pass A (or update), the stash and the partials beside it."""
        p = self._place_state(model)
        if self.small_omega is None:
            self.small_omega, self.omega, self.anchor = torch.zeros_like(p), torch.zeros_like(p), p.detach().clone()
        if self._stash_g is None:
            self._stash_g, self._stash_p = torch.empty_like(p), torch.empty_like(p)
            self._pen = torch.zeros_like(self._clip_partials(p, ops.si_blocks))
            self.last_penalty = torch.zeros(1, dtype=torch.float32, device=p.device)[0]

    # ---- between tasks -----------------------------------------------------------------------------------------------------
    def update(self, model, **kwargs) -> None:
        self._ensure(model)
        if self._pending:
            self.update_after_step(model=model)
        behind_optimizer(model)
        ops.si_consolidate_(model.flat_params, self.anchor, self.small_omega, self.omega, self.xi)
        self.task_id += 1

    # ---- inside a step -----------------------------------------------------------------------------------------------------
    def update_after_backward(self, model=None, **kwargs) -> None:
        """Pass A.  Trainer calls this only on the micro-batch that closes a window."""
        self._ensure(model)
        reg = self.task_id > 0
        ops.si_stash(model.flat_grads, model.flat_params, self.omega if reg else None, self.anchor if reg else None, 2.0 * float(self.reg_lambda),
                     self._stash_g, self._stash_p, self._partials, self._pen)
        if reg:
            ops.si_penalty_finish(self._pen, float(self.reg_lambda), self.last_penalty)
        self._hand_over(model)
        self._pending = True

    def update_after_step(self, model=None, **kwargs) -> None:
        """Pass B, behind the optimiser step that followed the pending pass A.  On the caller's stream, so the next pass A and
        ``update()`` are behind it by stream order."""
        self._native(model)
        if not self._pending:
            return
        self._pending = False
        behind_optimizer(model)
        ops.si_accumulate_(self._stash_g, self._stash_p, model.flat_params, self.small_omega)

    # ---- checkpoints between tasks -----------------------------------------------------------------------------------------
    def state_dict(self):
        return {**self._state_tensors(), "task_id": self.task_id}

    def load_state_dict(self, sd) -> None:
        self._require_keys(sd, ("task_id",))
        names = ("omega", "anchor", "small_omega")
        self._load_tensors(sd, () if any(sd[k] is None for k in names) else names)   # without one of them there is no state
        self._pending = False
        self.task_id = int(sd["task_id"])
