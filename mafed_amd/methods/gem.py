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
from mafed_amd.methods.flat import require_native
from mafed_amd.methods.memory import HBMReplayBuffer
from mafed_amd.methods.replay import ER

GEM_MAX_REFS = ops.GEM_MAX_REFS


class GEM(ER):
    """GEM.  The constructor arguments and the selection of ``update(dataset, model=...)`` are ER's (same rng stream, same stored
    samples); ``update`` also keeps one memory per finished task (``task_memories``), and the work is in ``update_after_backward``
    (Lightning's on_before_optimizer_step): 1 + K forward + backward per optimiser step by construction."""
    grads_only_through_model = False   # the projection rewrites the gradient buffer behind the model's backward: one-pass / handed-over clip norm
    single_process_only = True         # under DDP the projection would have to act on the reduced gradients (Trainer refuses a reducer)

    def __init__(self, opts, memory_size, model_type, margin: float = 0.5, eps: float = 1e-3, memory_selection=None, **kwargs):
        super().__init__(opts, memory_size, model_type, memory_selection=memory_selection, **kwargs)
        if margin < 0 or eps < 0:
            raise ValueError(f"GEM: margin and eps must be >= 0, got {margin} and {eps}")
        self.margin, self.eps = float(margin), float(eps)
        self.task_memories: List[HBMReplayBuffer] = []   # one per finished task, over that task's stored samples
        self._stash: Optional[torch.Tensor] = None       # g while flat_grads receives the reference gradients; allocated once
        self._refs: List[torch.Tensor] = []              # K - 1 scratch buffers (the last task's gradient stays in flat_grads)
        self._gram: Optional[torch.Tensor] = None        # device fp64 [(K + 1)^2], sized for the current K
        self._stats: Optional[torch.Tensor] = None       # device {v_0 .. v_7, violated, support size, 0, 0}
        self._partials: Optional[torch.Tensor] = None    # sum-of-squares partials of g~ for the clip norm
        # device views (no host synchronisation); None until the first projection
        self.last_gram = self.last_coef = self.last_violated = self.last_support = None

    _WHY_NATIVE = "the projection runs on its flat gradient buffer (model.flat_grads)"

    def update(self, dataset, model=None, **kwargs):
        if len(self.task_memories) >= GEM_MAX_REFS:   # (before anything of the plugin's has changed)
            raise RuntimeError(f"GEM: {GEM_MAX_REFS} finished tasks hold a constraint each and the solve takes no more "
                               f"(GEM_MAX_REFS = {GEM_MAX_REFS}); use AGEM for longer task sequences")
        if model is not None:
            require_native(model, "GEM", self._WHY_NATIVE)
        super().update(dataset, model=model, **kwargs)
        mixed = self.mem_dataloader
        mem = HBMReplayBuffer(self.batch_size, mixed.device, seed=self.opts.seed + 1 + len(self.task_memories),
                              feature_dtype=mixed.feature_dtype)
        mem.add(self.datasets[-1])
        self.task_memories.append(mem)

    def replay(self, model, **kwargs):
        """Never a replay step: the Trainer falls through to the task branch."""
        return None, 0

    def compute_loss(self, model, loss, **kwargs):
        return loss

    def _buffers(self, g: torch.Tensor, K: int) -> None:
        """The stash, the K - 1 scratch refs and the device scalars: allocated once, grown when a task has been added."""
        if self._stash is None or self._stash.shape != g.shape or self._stash.device != g.device:
            self._stash = torch.empty_like(g)
            self._refs = []
            self._stats = torch.zeros(12, dtype=torch.float32, device=g.device)
            self._partials = torch.zeros(ops.gem_blocks(g.numel()), dtype=torch.float32, device=g.device)
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
        require_native(model, "GEM", self._WHY_NATIVE)
        K = len(mems)
        self._buffers(model.flat_grads, K)
        self._stash.copy_(model.flat_grads)
        refs = []
        for k, mem in enumerate(mems):
            model.zero_grad()
            batch = next(iter(mem))
            model(**batch, compute_loss=True, return_dict=True).loss.backward()   # flat_grads now holds r_k
            if k < K - 1:
                refs.append(self._refs[k].copy_(model.flat_grads))
        out = model.flat_grads
        refs.append(out)
        ops.gem_gram(self._stash, refs, self._gram)
        ops.gem_solve(self._gram, K, self.margin, self.eps, self._stats)
        ops.gem_project(self._stash, refs, self._stats, out=out, sumsq_partials=self._partials)
        model.final_grad_sumsq = self._partials   # FlatAdamW.clip_grad_norm_ folds these instead of reading the buffer again
