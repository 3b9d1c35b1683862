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
from mafed_amd.methods.flat import FlatDict, behind_optimizer, require_native


class SI(CLStrategy):
    """``SI(reg_lambda=1.0, xi=1e-3)``.  ``xi`` damps the division where a parameter barely moved; 1e-3 is the paper's CIFAR value and has
    not been tuned for this model."""
    # grads_only_through_model stays False: pass A rewrites the gradient buffer behind the model's backward (handed-over clip norm)
    single_process_only = True         # under a reducer the hook runs before the reduced gradients exist (Trainer refuses one)

    def __init__(self, reg_lambda=1.0, xi=1e-3, **kwargs):
        super().__init__(reg_lambda, **{k: v for k, v in kwargs.items() if k in ("mask", "scaler", "opts")})
        if not xi > 0:
            raise ValueError("xi must be positive")
        self.xi = float(xi)
        self.small_omega: Optional[torch.Tensor] = None   # w: the running path integral of the task being learnt
        self.omega: Optional[torch.Tensor] = None         # consolidated importance
        self.anchor: Optional[torch.Tensor] = None        # parameters at the last consolidation (task 0: at the first pass A)
        self._stash_g = self._stash_p = self._sumsq = self._pen = None
        self.last_penalty: Optional[torch.Tensor] = None  # device scalar c sum Omega (p - p*)^2 of the last pass A; None until the first
        self._pending = False                             # a pass A whose pass B has not run yet

    # ---- buffers -----------------------------------------------------------------------------------------------------------
    def _native(self, model):
        require_native(model, "SI", "its passes run on the flat buffers (model.flat_params / model.flat_grads)")
        return model.flat_params

    def _ensure(self, model) -> None:
        """Allocate once: the state at the first pass A (or update), the stash and the partials beside it."""
        p = self._native(model)
        if self.small_omega is None:
            self.small_omega, self.omega, self.anchor = torch.zeros_like(p), torch.zeros_like(p), p.detach().clone()
        if self.small_omega.shape != p.shape:
            raise ValueError("SI's state was built for another model (%d elements, this one has %d)" % (self.small_omega.numel(), p.numel()))
        if self.small_omega.device != p.device:   # a checkpoint loaded on another device
            self.small_omega, self.omega, self.anchor = (t.to(p.device) for t in (self.small_omega, self.omega, self.anchor))
        if self._stash_g is None:
            self._stash_g, self._stash_p = torch.empty_like(p), torch.empty_like(p)
            nb = ops.si_blocks(p.numel())
            self._sumsq, self._pen = torch.zeros(nb, dtype=torch.float32, device=p.device), torch.zeros(nb, dtype=torch.float32, device=p.device)
            self.last_penalty = torch.zeros(1, dtype=torch.float32, device=p.device)[0]

    def named(self, model, which: str = "omega") -> FlatDict:
        """name -> view of ``omega`` / ``small_omega`` / ``anchor``, like EWC's ``fisher[0]``."""
        if which not in ("omega", "small_omega", "anchor"):
            raise KeyError(which)
        self._ensure(model)
        return FlatDict(model, getattr(self, which))

    _behind_optimizer = staticmethod(behind_optimizer)

    # ---- between tasks -----------------------------------------------------------------------------------------------------
    def update(self, model, **kwargs) -> None:
        self._ensure(model)
        if self._pending:
            self.update_after_step(model=model)
        self._behind_optimizer(model)
        ops.si_consolidate_(model.flat_params, self.anchor, self.small_omega, self.omega, self.xi)
        self.task_id += 1

    # ---- inside a step -----------------------------------------------------------------------------------------------------
    def compute_loss(self, model, loss, **kwargs):
        return loss

    def update_after_backward(self, model=None, **kwargs) -> None:
        """Pass A.  Trainer calls this only on the micro-batch that closes a window."""
        self._ensure(model)
        reg = self.task_id > 0
        ops.si_stash(model.flat_grads, model.flat_params, self.omega if reg else None, self.anchor if reg else None, 2.0 * float(self.reg_lambda),
                     self._stash_g, self._stash_p, self._sumsq, self._pen)
        if reg:
            ops.si_penalty_finish(self._pen, float(self.reg_lambda), self.last_penalty)
        model.final_grad_sumsq = self._sumsq   # FlatAdamW.clip_grad_norm_ folds these instead of reading the buffer again
        self._pending = True

    def update_after_step(self, model=None, **kwargs) -> None:
        """Pass B, behind the optimiser step that followed the pending pass A.  On the caller's stream, so the next pass A and
        ``update()`` are behind it by stream order."""
        self._native(model)
        if not self._pending:
            return
        self._pending = False
        self._behind_optimizer(model)
        ops.si_accumulate_(self._stash_g, self._stash_p, model.flat_params, self.small_omega)

    # ---- checkpoints between tasks -----------------------------------------------------------------------------------------
    def state_dict(self):
        return {"omega": self.omega, "anchor": self.anchor, "small_omega": self.small_omega, "task_id": self.task_id}

    def load_state_dict(self, sd) -> None:
        missing = [k for k in ("omega", "anchor", "small_omega", "task_id") if k not in sd]
        if missing:
            raise ValueError("SI state without %s" % missing)
        if any(sd[k] is None for k in ("omega", "anchor", "small_omega")):
            self.small_omega = self.omega = self.anchor = None
        else:
            self.omega, self.anchor, self.small_omega = (sd[k].detach().to(torch.float32).clone().contiguous() for k in ("omega", "anchor", "small_omega"))
        self._pending = False
        self.task_id = int(sd["task_id"])
