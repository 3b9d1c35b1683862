"""Learning without Forgetting (Li & Hoiem, 2016) for the answer tokens of the VQA batches: a memory-free plugin.

The reference ships no implementation (its tooling only knows the checkpoint suffix ``_lwf``, mafed/utils/eval_utils.py:23), so the
arithmetic is this project's: while task k > 0 is learnt, the model of task k-1 -- a frozen snapshot, as in
``FeatureDistillation._update_model`` -- scores the CURRENT batch, and the head loss becomes

    loss = CE + reg_lambda * temperature^2 * KL(softmax(t / temperature) || softmax(s / temperature))

over the rows that carry a label, normalised like the cross-entropy.  The term lives inside the model's own step: ``update`` puts a
``LogitDistillation`` into ``model.head_loss``, the engine asks it for the teacher's logits on the rows its head runs on and the fused
kernels of ``csrc/kd.hip`` do the rest, so the step stays one autograd node and every parameter gradient comes out of the model's sweep.
"""
from __future__ import annotations

from copy import deepcopy
from typing import Optional

import torch

from mafed_amd.head_loss import LogitDistillation
from mafed_amd.methods.base import CLStrategy


class LwF(CLStrategy):
    """Answer-token logit distillation from the previous task's model.  ``reg_lambda`` weighs the term, ``temperature`` softens both
    distributions.  No replay memory: ``replay`` is the base no-op."""
    grads_only_through_model = True  # every parameter gradient of a step comes out of the model's own backward (Trainer: incremental clip norm)

    def __init__(self, opts=None, reg_lambda: float = 1.0, temperature: float = 2.0, **kwargs):
        super().__init__(reg_lambda=reg_lambda, opts=opts, **{k: v for k, v in kwargs.items() if k in ("mask", "scaler")})
        if not temperature > 0:
            raise ValueError(f"temperature must be positive, not {temperature!r}")
        self.temperature = float(temperature)
        self.opts = opts
        self.past_model = None
        self.last_ce: Optional[torch.Tensor] = None   # device scalars of the last compute_loss (no host synchronisation)
        self.last_kd: Optional[torch.Tensor] = None

    # ---- between tasks -----------------------------------------------------------------------------------------------
    def update(self, model, **kwargs):
        """Teacher := frozen copy of the finished task's model; from now on the model's training head loss carries the KL term."""
        if not hasattr(model, "head_logits_rows"):
            raise TypeError("LwF needs the native model: the distillation term is computed inside its head (model.head_loss)")
        self.past_model = deepcopy(model)   # (VLPythiaForCausalLM.__deepcopy__: the frozen vision tower is shared; the copy's head_loss is empty)
        self.past_model.eval()
        for p in self.past_model.parameters():
            p.requires_grad_(False)
        model.head_loss = LogitDistillation(self._teacher_logits)
        self.task_id += 1

    def _teacher_logits(self, feats, input_ids, attention_mask, rows):
        """The teacher of ``LogitDistillation``: the frozen model's logits on the text rows the student's head runs on (None = all) + (tau, lambda)."""
        return self.past_model.head_logits_rows(feats, input_ids, attention_mask, rows), self.temperature, float(self.reg_lambda)

    # ---- inside a step ---------------------------------------------------------------------------------------------------
    def compute_loss(self, model, loss, batch=None, **kwargs):
        """The term is already inside ``loss`` (the model's head computed CE + lambda tau^2 KL): returned unchanged.  ``last_ce`` /
        ``last_kd`` are the two parts of the step, for logging."""
        if self.task_id > 0 and isinstance(model.head_loss, LogitDistillation):   # (task 0: any model, plain cross-entropy)
            self.last_ce, self.last_kd = model.last_head_losses[1], model.last_head_losses[2]
        else:
            self.last_ce = loss.detach()
            self.last_kd = model._hook_zero().view(()) if hasattr(model, "_hook_zero") else torch.zeros((), device=loss.device)
        return loss
