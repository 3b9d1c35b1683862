"""Memory Aware Synapses (Aljundi et al. 2018): the regulariser whose importance is the sensitivity of the model's output, not of its loss.

The reference ships no implementation, so the arithmetic is this project's.  The state is two flat fp32 buffers
laid out like ``model.flat_params``: the importance Omega (``omega``) and the anchor p* (``anchor``), 8 bytes per parameter; a third, the
accumulator, lives only while an importance pass runs.  With c = ``reg_lambda`` and a = ``alpha``:

    update  between tasks, over a dataloader of the task just learnt
            per batch of n samples:  zero_grad, forward with the squared-norm head objective J (``model.head_loss = SquaredNorm()``:
            mean_b of sum_t |logits[b,t]|^2 / count_b over the answer rows -- the label values are never read), backward,
            acc += n |g|;  then  Omega_new = acc / N,  Omega = Omega_new (first task) or a Omega + (1 - a) Omega_new,  p* = p,
            task_id += 1
    step    update_after_backward, on the micro-batch that closes a window, in front of the clip, from task 1 on
            g += 2c Omega (p - p*)  in place; leaves the clip's sum-of-squares partials of the g it leaves
            (``model.final_grad_sumsq``) and ``last_penalty`` = c sum Omega (p - p*)^2

|g| is the absolute value of the batch-mean gradient, as Avalanche's MAS takes it; a loader of batch size 1 gives the paper's
per-sample form.  The penalty never enters autograd -- ``compute_loss`` returns the loss unchanged -- so its gradient is added once per
window, after the last backward, whatever the backward did to the gradient buffer before (overwriting weight-gradient sweeps included).
On task 0 the plugin does nothing inside a step.  Nothing here synchronises with the host.  The passes are ``csrc/mas.hip``, the head
objective ``csrc/sqnorm.hip``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from mafed_amd import ops
from mafed_amd.head_loss import SquaredNorm
from mafed_amd.methods.base import CLStrategy
from mafed_amd.methods.flat import FlatDict, FlatPlugin, behind_optimizer


class MAS(FlatPlugin, CLStrategy):
    """``MAS(reg_lambda=1.0, alpha=0.5)``.  ``alpha`` weighs the old importance against the new one at a task boundary (0.5 is Avalanche's
    default); neither it nor ``reg_lambda`` has been tuned for this model."""
    _STATE = (("omega", torch.float32), ("anchor", torch.float32))

    def __init__(self, reg_lambda=1.0, alpha=0.5, **kwargs):
        super().__init__(reg_lambda, **{k: v for k, v in kwargs.items() if k in ("mask", "scaler", "opts")})
        if not 0.0 <= alpha <= 1.0:
            raise ValueError("alpha must lie in [0, 1]")
        self.alpha = float(alpha)
        self.omega: Optional[torch.Tensor] = None         # consolidated importance; None until the first update
        self.anchor: Optional[torch.Tensor] = None        # parameters at the last consolidation
        self._pen = None
        self.last_penalty: Optional[torch.Tensor] = None  # device scalar c sum Omega (p - p*)^2 of the last penalty pass; None until the first

    # ---- buffers -----------------------------------------------------------------------------------------------------------
    def _ensure(self, model) -> None:
        """Allocate once: the state and the partials, at the first update (or the first penalty pass after a checkpoint)."""
        p = self._place_state(model)
        if self.omega is None:
            self.omega, self.anchor = torch.zeros_like(p), p.detach().clone()
        if self._pen is None:
            self._pen = torch.zeros_like(self._clip_partials(p, ops.mas_blocks))
            self.last_penalty = torch.zeros(1, dtype=torch.float32, device=p.device)[0]

    # ---- between tasks -----------------------------------------------------------------------------------------------------
    def _importance_sums(self, model, dataloader) -> Tuple[torch.Tensor, float]:
        """(acc = sum over batches of n |grad J|, N = samples seen).  What ``model.head_loss`` held is put back whatever happens."""
        p = self._native(model)
        if dataloader is None:
            raise ValueError("MAS needs the dataloader of the task just learnt to measure the importance")
        model.train()
        behind_optimizer(model)   # (zero_grad below writes the buffer a pipelined update may still be zeroing)
        acc, seen = torch.zeros_like(p), 0
        previous, model.head_loss = model.head_loss, SquaredNorm()
        try:
            for batch in dataloader:
                model.zero_grad()
                n = batch["input_ids"].size(0)
                model(**batch, compute_loss=True, return_dict=True).loss.backward()
                ops.mas_accumulate_(model.flat_grads, acc, float(n))
                seen += n
        finally:
            model.head_loss = previous
            model.zero_grad()
        if seen == 0:
            raise ValueError("MAS: the importance dataloader is empty")
        return acc, float(seen)

    def compute_importances(self, model, dataloader) -> FlatDict:
        """Omega_new = sum over batches of n |grad J| / N: the absolute value of each batch's mean gradient of the squared-norm objective,
        weighted by the batch size."""
        acc, seen = self._importance_sums(model, dataloader)
        return FlatDict(model, acc.mul_(1.0 / seen))

    def update(self, model, dataloader=None, **kwargs) -> None:
        acc, seen = self._importance_sums(model, dataloader)
        first = self.omega is None or self.task_id == 0
        self._ensure(model)
        behind_optimizer(model)
        ops.mas_consolidate_(acc, self.omega, model.flat_params, self.anchor, 1.0 / seen, self.alpha, first)
        self.task_id += 1   # (acc is dropped here: the state is omega and anchor)

    # ---- inside a step -----------------------------------------------------------------------------------------------------
    def update_after_backward(self, model=None, **kwargs) -> None:
        """The penalty pass.  Trainer calls this only on the micro-batch that closes a window; on task 0 it does nothing."""
        self._native(model)
        if self.task_id == 0 or self.omega is None:
            return
        self._ensure(model)
        c = float(self.reg_lambda)
        ops.mas_penalty_(model.flat_grads, model.flat_params, self.omega, self.anchor, 2.0 * c, self._partials, self._pen)
        ops.si_penalty_finish(self._pen, c, self.last_penalty)
        self._hand_over(model)

    # ---- checkpoints between tasks -----------------------------------------------------------------------------------------
    def state_dict(self):
        return {**self._state_tensors(), "task_id": self.task_id}

    def load_state_dict(self, sd) -> None:
        self._require_keys(sd, ("task_id",))
        names = ("omega", "anchor")
        self._load_tensors(sd, () if any(sd[k] is None for k in names) else names)   # without one of them there is no state
        self.task_id = int(sd["task_id"])
