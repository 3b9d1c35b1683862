"""Gradient Episodic Memory (Lopez-Paz & Ranzato, 2017): one gradient constraint per finished task, on ER's replay memory.

A-GEM (``mafed_amd.AGEM``) is this method's averaged relaxation.  The reference ships no implementation, so the arithmetic is this
project's.  On the micro-batch that closes an accumulation window, between the backward and the clip, the
window's gradient g is compared with the gradients r_1 .. r_K of the model's ordinary loss on one memory batch of each finished task
(K <= 8), at the same parameters:

    gram[a][b] = sum x_a x_b (x_0 = g, x_k = r_k; fp64)    q_k = gram[0][k]    P = gram[1..K][1..K] + eps I
    every q_k >= 0:  g stays as it is.    Else  v = argmin 1/2 v'Pv + q'v  s.t. v_k >= margin,  g~ = g + sum_k v_k r_k

and g~ goes on to clip, optimiser and scheduler.  The Gram, the exact solve and the K-term AXPY are the three entry points of
``csrc/gem.hip``; the Gram, v, the violated flag and the support size stay on the device.  ``margin`` and ``eps`` default to the
published implementation's 0.5 and 1e-3 and are untuned for this model.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from mafed_amd import ops
from mafed_amd.methods.agem import MemoryProjection
from mafed_amd.methods.memory import HBMReplayBuffer

GEM_MAX_REFS = ops.GEM_MAX_REFS


class GEM(MemoryProjection):
    """GEM.  The constructor arguments and the selection of ``update(dataset, model=...)`` are ER's (same rng stream, same stored
    samples); ``update`` also keeps one memory per finished task (``task_memories``), and the work is in ``update_after_backward``
    (Lightning's on_before_optimizer_step): 1 + K forward + backward per optimiser step by construction."""

    def __init__(self, opts, memory_size, model_type, margin: float = 0.5, eps: float = 1e-3, memory_selection=None, **kwargs):
        super().__init__(opts, memory_size, model_type, memory_selection=memory_selection, **kwargs)
        if margin < 0 or eps < 0:
            raise ValueError(f"GEM: margin and eps must be >= 0, got {margin} and {eps}")
        self.margin, self.eps = float(margin), float(eps)
        self.task_memories: List[HBMReplayBuffer] = []   # one per finished task, over that task's stored samples
        self._refs: List[torch.Tensor] = []              # K - 1 scratch buffers (the last task's gradient stays in flat_grads)
        self._gram: Optional[torch.Tensor] = None        # device fp64 [(K + 1)^2], sized for the current K
        self._stats: Optional[torch.Tensor] = None       # device {v_0 .. v_7, violated, support size, 0, 0}
        # device views (no host synchronisation); None until the first projection
        self.last_gram = self.last_coef = self.last_violated = self.last_support = None

    def update(self, dataset, model=None, **kwargs):
        if len(self.task_memories) >= GEM_MAX_REFS:   # (before anything of the plugin's has changed)
            raise RuntimeError(f"GEM: {GEM_MAX_REFS} finished tasks hold a constraint each and the solve takes no more "
                               f"(GEM_MAX_REFS = {GEM_MAX_REFS}); use AGEM for longer task sequences")
        super().update(dataset, model=model, **kwargs)
        mixed = self.mem_dataloader
        mem = HBMReplayBuffer(self.batch_size, mixed.device, seed=self.opts.seed + 1 + len(self.task_memories),
                              feature_dtype=mixed.feature_dtype)
        mem.add(self.datasets[-1])
        self.task_memories.append(mem)

    def _buffers(self, model, K: int) -> None:
        """The K - 1 scratch refs and the device scalars beside the stash: allocated once, grown when a task has been added."""
        new = self._new_buffers(model, ops.gem_blocks)
        g = model.flat_grads
        if new:
            self._refs = []
            self._stats = torch.zeros(12, dtype=torch.float32, device=g.device)
            self.last_coef, self.last_violated, self.last_support = self._stats[:GEM_MAX_REFS], self._stats[8], self._stats[9]
            self._gram = None
        while len(self._refs) < K - 1:
            self._refs.append(torch.empty_like(g))
        if self._gram is None or self._gram.numel() != (K + 1) * (K + 1):
            self._gram = torch.zeros((K + 1, K + 1), dtype=torch.float64, device=g.device)
            self.last_gram = self._gram

    def update_after_backward(self, model=None, **kwargs) -> None:
        mems = [m for m in self.task_memories if len(m)]
        if self.task_id == 0 or not mems:
            return
        K = len(mems)
        self._buffers(model, K)
        refs = []

        def keep(k):
            if k < K - 1:
                refs.append(self._refs[k].copy_(model.flat_grads))
        self._memory_gradients(model, mems, keep)
        out = model.flat_grads   # (the last task's gradient stays where the backward left it)
        refs.append(out)
        ops.gem_gram(self._stash, refs, self._gram)
        ops.gem_solve(self._gram, K, self.margin, self.eps, self._stats)
        ops.gem_project(self._stash, refs, self._stats, out=out, sumsq_partials=self._partials)
        self._hand_over(model)
