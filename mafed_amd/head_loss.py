"""The loss the LM head takes on a training forward with labels: one object in ``model.head_loss`` (None = cross-entropy).

The engine (engine.py: ``_head_loss``) calls ``prepare`` in front of the head GEMM and ``forward`` behind it.  The objects keep nothing
between forwards: what one forward's backward needs travels in the closure that forward returns, which the backward sweep pops and calls
once.  Every ``ops.<name>`` is looked up on the module when it is called, so a test or tool that replaces one sees its replacement run.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch

from mafed_amd import ops

# (logits, head labels, gloss [1]) -> dlogits
Backward = Callable[[torch.Tensor, torch.Tensor, torch.Tensor], torch.Tensor]


class HeadLoss:
    def prepare(self, feats, input_ids, attention_mask, rows):
        """In front of the head GEMM, on the caller's stream: the padded batch of this forward and the head's row selection (the row-sparse
        head's ``row_of_slot`` [B * Rc] int32, or None = all T text rows) -> whatever ``forward`` wants back as ``prepared``."""
        return None

    def forward(self, logits, labels, poison, prepared) -> Tuple[torch.Tensor, Optional[torch.Tensor], Backward]:
        """Head logits [B, R, V], the head's own labels [B, R] (dense or compact) and the row-sparse head's overflow flag (or None) ->
        (loss [1], parts = the device [3] tensor for ``model.last_head_losses`` or None, backward)."""
        raise NotImplementedError


class CrossEntropy(HeadLoss):
    def forward(self, logits, labels, poison, prepared):
        loss, lse = ops.ce_fwd(logits, labels, poison=poison)
        return loss, None, lambda lg, lab, gl: ops.ce_bwd(lg, lab, lse, gl)


CROSS_ENTROPY = CrossEntropy()   # the loss of an empty slot


class SquaredNorm(HeadLoss):
    """Mean over samples of sum_t |logits[b,t]|^2 / count_b on the labelled rows: the objective of the MAS importance pass."""

    def forward(self, logits, labels, poison, prepared):
        loss, _ = ops.sqnorm_fwd(logits, labels, poison=poison)
        return loss, None, lambda lg, lab, gl: ops.sqnorm_bwd(lg, lab, gl)


class LogitDistillation(HeadLoss):
    """CE + lambda tau^2 KL against a teacher's logits of the same rows, one pass.  ``teacher`` is a callable
    (feats, input_ids, attention_mask, rows) -> (teacher logits in compute dtype, tau, lambda), asked once per forward."""

    def __init__(self, teacher):
        self.teacher = teacher

    def prepare(self, feats, input_ids, attention_mask, rows):
        t_logits, tau, lam = self.teacher(feats, input_ids, attention_mask, rows)
        return t_logits.detach(), float(tau), float(lam)

    def forward(self, logits, labels, poison, prepared):
        t_logits, tau, lam = prepared
        if t_logits.dtype != logits.dtype or t_logits.numel() != logits.numel():
            raise ValueError(f"the logit teacher returned {tuple(t_logits.shape)} {t_logits.dtype} for head rows {tuple(logits.shape)} {logits.dtype}")
        t_logits = t_logits.contiguous().view(logits.shape)
        out3, lse3 = ops.ce_kd_fwd(logits, t_logits, labels, tau, lam, poison=poison)
        return out3[0:1], out3, lambda lg, lab, gl: ops.ce_kd_bwd(lg, t_logits, lab, lse3, tau, lam, gl)


class LogitAnchor(HeadLoss):
    """beta CE + alpha MSE against stored logits, read in place: labelled row (b, t) is held against
    ``store[mem_index[b], rank of t among b's labelled rows]``; the rank is the same under dense and compact labels.  ``store``
    [n_mem, A, V] in compute dtype, ``mem_index`` int64 [B]; both are checked at the forward (ops._anchor_args), not here."""

    def __init__(self, store, mem_index, alpha, beta):
        self.store, self.mem_index, self.alpha, self.beta = store, mem_index, alpha, beta

    def forward(self, logits, labels, poison, prepared):
        store, mem_index, alpha, beta = self.store, self.mem_index, float(self.alpha), float(self.beta)
        if not torch.is_tensor(store) or not torch.is_tensor(mem_index):
            raise ValueError(f"LogitAnchor: store and mem_index must be tensors, got {type(store).__name__} and {type(mem_index).__name__}")
        store, mem_index = store.detach(), mem_index.to(logits.device).contiguous()
        out3, lse = ops.ce_mse_fwd(logits, store, mem_index, labels, alpha, beta, poison=poison)
        return out3[0:1], out3, lambda lg, lab, gl: ops.ce_mse_bwd(lg, store, mem_index, lab, lse, alpha, beta, gl)
