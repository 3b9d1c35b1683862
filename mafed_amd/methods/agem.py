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

from typing import Callable, Iterable, Optional

import torch

from mafed_amd import ops
from mafed_amd.methods.flat import FlatPlugin
from mafed_amd.methods.replay import ER


class MemoryProjection(FlatPlugin, ER):
    """What A-GEM and GEM share: the memory, the constructor arguments and ``update(dataset, model=...)`` are ER's; the work is in the
    subclass's ``update_after_backward`` (Lightning's on_before_optimizer_step), which compares the window's gradient with gradients
    of the model's ordinary loss on memory batches and leaves the projected gradient in ``flat_grads``."""
    # (ER's grads_only_through_model is True; FlatPlugin's False is in front of it)
    _WHY_NATIVE = "the projection runs on its flat gradient buffer (model.flat_grads)"
    _stash: Optional[torch.Tensor] = None   # g while flat_grads receives the memory gradients; allocated once

    def update(self, dataset, model=None, **kwargs):
        if model is not None:
            self._native(model)
        super().update(dataset, model=model, **kwargs)

    def replay(self, model, **kwargs):
        """Never a replay step: the Trainer falls through to the task branch."""
        return None, 0

    def _new_buffers(self, model, blocks: Callable[[int], int]) -> bool:
        """The stash and the clip partials of the projected gradient: allocated once.  True when they are new (the first projection, or
        another gradient buffer), for the subclass to allocate its own beside them."""
        self._native(model)
        g = model.flat_grads
        if self._stash is not None and self._stash.shape == g.shape and self._stash.device == g.device:
            return False
        self._stash, self._partials = torch.empty_like(g), None
        self._clip_partials(g, blocks)
        return True

    def _memory_gradients(self, model, loaders: Iterable, then: Optional[Callable[[int], None]] = None) -> None:
        """g goes to the stash; then one batch of every loader in turn leaves its gradient in ``flat_grads``, and ``then(k)`` runs
        behind the k-th backward."""
        self._stash.copy_(model.flat_grads)
        for k, loader in enumerate(loaders):
            model.zero_grad()
            batch = next(iter(loader))
            model(**batch, compute_loss=True, return_dict=True).loss.backward()   # flat_grads now holds r_k
            if then is not None:
                then(k)


class AGEM(MemoryProjection):
    """A-GEM: one reference gradient, from a batch of the mixed memory."""

    def __init__(self, opts, memory_size, model_type, **kwargs):
        super().__init__(opts, memory_size, model_type, **kwargs)
        self._stats: Optional[torch.Tensor] = None      # device {dot, rsq, alpha, violated} of the last projection
        # views of ``_stats`` (no host synchronisation); None until the first projection
        self.last_dot = self.last_ref_sq = self.last_alpha = self.last_projected = None

    def update_after_backward(self, model=None, **kwargs) -> None:
        if self.task_id == 0 or self.mem_dataloader is None or len(self.mem_dataloader) == 0:
            return
        if self._new_buffers(model, ops.agem_blocks):
            self._stats = torch.zeros(4, dtype=torch.float32, device=model.flat_grads.device)
            self.last_dot, self.last_ref_sq, self.last_alpha, self.last_projected = (self._stats[i] for i in range(4))
        self._memory_gradients(model, [self.mem_dataloader])
        r = model.flat_grads
        ops.agem_dots(self._stash, r, self._stats)
        ops.agem_project(self._stash, r, self._stats, out=r, sumsq_partials=self._partials)
        self._hand_over(model)
