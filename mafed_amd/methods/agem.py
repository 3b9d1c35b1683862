"""Averaged GEM (Chaudhry et al., 2019): the gradient-constraint baseline on ER's replay memory.

The reference ships no implementation (its tooling only knows the checkpoint suffix ``_agem``, mafed/utils/eval_utils.py:23), so the
arithmetic is this project's.  On the micro-batch that closes an accumulation window, between the backward and
the clip, the window's gradient g is compared with the gradient r of the model's ordinary loss on one memory batch at the same
parameters:

    dot = sum g r    rsq = sum r r    alpha = dot / rsq if dot < 0 and rsq > 0, else 0    g' = g - alpha r

and g' goes on to clip, optimiser and scheduler.  The task batch is never swapped for a memory batch.  Both reductions and the AXPY run
over the flat gradient buffer in two passes of ``csrc/agem.hip``; dot, rsq, alpha and the violated flag stay on the device.
"""
from __future__ import annotations

from typing import Optional

import torch

from mafed_amd import ops
from mafed_amd.methods.flat import require_native
from mafed_amd.methods.replay import ER


class AGEM(ER):
    """A-GEM.  The memory, the constructor arguments and ``update(dataset, model=...)`` are ER's; the work is in
    ``update_after_backward`` (Lightning's on_before_optimizer_step)."""
    grads_only_through_model = False   # (ER's is True) the projection rewrites the gradient buffer behind the model's backward: one-pass / handed-over clip norm
    single_process_only = True         # under DDP the projection would have to act on the reduced gradients (Trainer refuses a reducer)

    def __init__(self, opts, memory_size, model_type, **kwargs):
        super().__init__(opts, memory_size, model_type, **kwargs)
        self._stash: Optional[torch.Tensor] = None      # g while flat_grads receives r; allocated once
        self._stats: Optional[torch.Tensor] = None      # device {dot, rsq, alpha, violated} of the last projection
        self._partials: Optional[torch.Tensor] = None   # sum-of-squares partials of g' for the clip norm
        # views of ``_stats`` (no host synchronisation); None until the first projection
        self.last_dot = self.last_ref_sq = self.last_alpha = self.last_projected = None

    _WHY_NATIVE = "the projection runs on its flat gradient buffer (model.flat_grads)"

    def update(self, dataset, model=None, **kwargs):
        if model is not None:
            require_native(model, "AGEM", self._WHY_NATIVE)
        super().update(dataset, model=model, **kwargs)

    def replay(self, model, **kwargs):
        """Never a replay step: the Trainer falls through to the task branch."""
        return None, 0

    def compute_loss(self, model, loss, **kwargs):
        return loss

    def update_after_backward(self, model=None, **kwargs) -> None:
        if self.task_id == 0 or self.mem_dataloader is None or len(self.mem_dataloader) == 0:
            return
        require_native(model, "AGEM", self._WHY_NATIVE)
        g = model.flat_grads
        if self._stash is None or self._stash.shape != g.shape or self._stash.device != g.device:
            self._stash = torch.empty_like(g)
            self._stats = torch.zeros(4, dtype=torch.float32, device=g.device)
            self._partials = torch.zeros(ops.agem_blocks(g.numel()), dtype=torch.float32, device=g.device)
            self.last_dot, self.last_ref_sq, self.last_alpha, self.last_projected = (self._stats[i] for i in range(4))
        self._stash.copy_(g)
        model.zero_grad()
        batch = next(iter(self.mem_dataloader))
        model(**batch, compute_loss=True, return_dict=True).loss.backward()   # flat_grads now holds r
        r = model.flat_grads
        ops.agem_dots(self._stash, r, self._stats)
        ops.agem_project(self._stash, r, self._stats, out=r, sumsq_partials=self._partials)
        model.final_grad_sumsq = self._partials   # FlatAdamW.clip_grad_norm_ folds these instead of reading the buffer again
