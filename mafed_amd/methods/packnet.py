"""PackNet (Mallya & Lazebnik 2018): parameter isolation -- every task owns a disjoint subset of the weights, so nothing is forgotten.

The reference ships no implementation, so the arithmetic is this project's.  The state is two flat buffers laid out
like ``model.flat_params``: the byte-wide owner map (``owner``, the task that trained each element; all zero at first) and the fp32
``anchor`` (allocated at the first prune), 5 bytes per parameter.  One rule holds in every step of task t: element i is *trainable* iff
``owner[i] == t``.  Every other element is *held*:

    mask    update_after_backward, on the micro-batch that closes a window, in front of the clip
            g = owner == t ? g : +0.0  in place; leaves the clip's sum-of-squares partials of the g it leaves (``model.final_grad_sumsq``)
    hold    update_after_step, behind the optimiser, when a mask pass is pending
            where owner != t:  p = anchor, shadow = bf16(anchor)      (AdamW's decoupled decay moves a weight whose gradient is zero)
    prune   between or inside tasks, at most once per task, per prunable tensor:  m = #{owner == t},  k = floor(prune_fraction m),
            tau = the k-th smallest |p| among them;  where owner == t and |p| <= tau:  p = anchor = +0.0, shadow = 0, owner = t + 1
    update  between tasks:  prune first if the task has not been pruned;  anchor = p;  task_id += 1

The held elements are the frozen weights of earlier tasks (owner < t, anchor = their final value), the slots pruned in this task
(owner == t + 1, anchor = 0, while the task retrains) and the tensors that are never pruned (owner == 0 for good: trained on task 0, frozen
afterwards, as PackNet treats biases and norms).  While ``task_id == 0`` and nothing has been pruned every element is trainable, the plugin
launches nothing in a step and the run is Naive's bit for bit.  ``task_view(model, k)`` zeroes what tasks after k own and so gives back the model as it
stood right after task k's ``update``.  Nothing here synchronises with the host but ``prune_report``.  The passes are ``csrc/packnet.hip``.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, List, Optional

import torch

from mafed_amd import ops
from mafed_amd.methods.base import CLStrategy
from mafed_amd.methods.flat import FlatPlugin, behind_optimizer

MAX_TASKS = 255   # the owner map is a byte and a prune in task t writes t + 1


class PackNet(FlatPlugin, CLStrategy):
    """``PackNet(prune_fraction=0.5, prunable=None)``.  ``prune_fraction`` of a task's free weights goes to the next task at each prune
    (0.5 is the lowest setting of the paper; it is untuned for this model).  ``prunable``: callable(name) -> bool choosing the tensors
    that are pruned; default: the four weight matrices of every decoder layer."""
    # grads_only_through_model is False for the class: the mask pass rewrites the gradient buffer behind the model's backward (handed-over
    # clip norm).  An instance makes the promise while it launches nothing -- task 0 before its prune -- so that Trainer, which reads it
    # step by step, lets the sweep collect the clip norm as it does for Naive: the run is then Naive's whatever the clip does.
    _STATE = (("owner", torch.uint8), ("anchor", torch.float32))

    def __init__(self, prune_fraction=0.5, prunable: Optional[Callable[[str], bool]] = None, **kwargs):
        super().__init__(**{k: v for k, v in kwargs.items() if k in ("reg_lambda", "mask", "scaler", "opts")})
        if not 0.0 <= prune_fraction <= 1.0:
            raise ValueError("prune_fraction must lie in [0, 1]")
        self.prune_fraction = float(prune_fraction)
        self.prunable = prunable
        self.owner: Optional[torch.Tensor] = None     # uint8: the task that trained each element; None = all zero, not allocated yet
        self.anchor: Optional[torch.Tensor] = None    # fp32: what a held element is put back to; None until the first prune
        self.pruned = False                           # the current task has been pruned
        self.last_prune_stats: Optional[torch.Tensor] = None   # device int64 [tensors, 4] = {m, k, pruned, pattern of tau} of the last prune
        self._pending = False                         # a mask pass whose hold pass has not run yet
        self._promise()

    # ---- buffers -----------------------------------------------------------------------------------------------------------
    def _ensure(self, model) -> None:
        """Allocate once: the owner map and the mask pass's partials."""
        p = self._place_state(model)
        if self.owner is None:
            self.owner = torch.zeros(p.numel(), dtype=torch.uint8, device=p.device)
        self._clip_partials(p, ops.packnet_blocks)

    def prunable_names(self, model) -> List[str]:
        """The tensors a prune selects in, in the order of the flat layout."""
        self._native(model)
        if self.prunable is not None:
            return [name for name in model._offsets if self.prunable(name)]
        ranges = [model.layer_matrix_range(i) for i in range(model.config.num_hidden_layers)]
        return [name for name, (o, n, _) in model._offsets.items() if any(lo <= o and o + n <= hi for lo, hi in ranges)]

    # ---- between tasks -----------------------------------------------------------------------------------------------------
    def prune(self, model) -> None:
        """Hand ``prune_fraction`` of the current task's weights, the smallest in magnitude of each prunable tensor, to the next task."""
        self._ensure(model)
        if self._in_view:
            raise RuntimeError("PackNet: no prune inside a task_view")
        if self.pruned:
            raise RuntimeError("PackNet: task %d has been pruned already (one prune per task)" % self.task_id)
        if self.task_id + 1 > MAX_TASKS:
            raise RuntimeError("PackNet's owner map is a byte: %d tasks at most" % MAX_TASKS)
        if self._pending:
            self.update_after_step(model=model)
        behind_optimizer(model)
        if self.anchor is None:
            self.anchor = torch.zeros_like(model.flat_params)   # (read only where owner != task_id: written by this prune or by update)
        segments, (blocks, state, hist) = self._segment_tables(model, self.prunable_names(model), ops.packnet_select_blocks)   # (built here first)
        self.last_prune_stats = ops.packnet_prune_(model.flat_params, model.flat_shadow, self.owner, self.anchor, segments, blocks, self.task_id,
                                                   self.prune_fraction, state=state, hist=hist)
        self.pruned = True
        self._promise()

    def prune_report(self, model) -> Dict[str, Dict[str, int]]:
        """name -> {m, k, pruned, tau_bits} of the last prune.  The one call of this plugin that synchronises."""
        self._native(model)
        if self.last_prune_stats is None:
            return {}
        rows = self.last_prune_stats.cpu().tolist()
        return {name: dict(zip(("m", "k", "pruned", "tau_bits"), row)) for name, row in zip(self._segment_names, rows)}

    def update(self, model, **kwargs) -> None:
        self._ensure(model)
        if self._in_view:
            raise RuntimeError("PackNet: no update inside a task_view")
        if self.task_id + 1 >= MAX_TASKS:
            raise RuntimeError("PackNet's owner map is a byte: %d tasks at most" % MAX_TASKS)
        if not self.pruned:
            self.prune(model)
        if self._pending:
            self.update_after_step(model=model)
        behind_optimizer(model)
        self.anchor.copy_(model.flat_params)   # (the slots pruned in this task are 0 in both already)
        self.pruned = False
        self.task_id += 1
        self._promise()

    # ---- inside a step -----------------------------------------------------------------------------------------------------
    def _all_trainable(self) -> bool:
        return self.task_id == 0 and not self.pruned

    def _promise(self) -> None:
        self.grads_only_through_model = self._all_trainable()

    def update_after_backward(self, model=None, **kwargs) -> None:
        """The mask pass.  Trainer calls this only on the micro-batch that closes a window."""
        self._native(model)
        if self._in_view:
            raise RuntimeError("PackNet: no training step inside a task_view (the parameters are a view of task k, not the model)")
        if self._all_trainable():
            return
        self._ensure(model)
        ops.packnet_mask_grad_(model.flat_grads, self.owner, self.task_id, self._partials)
        self._hand_over(model)
        self._pending = True

    def update_after_step(self, model=None, **kwargs) -> None:
        """The hold pass, behind the optimiser step that followed the pending mask pass.  On the caller's stream: the next forward reads
        what it wrote by stream order, so a pipelined optimiser loses its overlap with that forward from task 1 on."""
        self._native(model)
        if not self._pending:
            return
        self._pending = False
        behind_optimizer(model)
        ops.packnet_hold_(model.flat_params, model.flat_shadow, self.owner, self.anchor, self.task_id)

    # ---- inference as of task k --------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def task_view(self, model, k: int):
        """Inside the block the model is the one that stood right after task k's ``update``: what tasks after k own is zero (every weight
        owned by a task <= k is frozen since).  ``0 <= k <=`` the number of finished tasks; that number itself gives the current weights.
        On exit the parameters and the shadow are put back bit for bit."""
        p = self._native(model)

        def prepare():
            if not 0 <= int(k) <= self.task_id:
                raise ValueError("task_view: k = %r outside 0 .. %d (the tasks finished so far)" % (k, self.task_id))
            if self._pending:
                self.update_after_step(model=model)

        def apply():
            if self.owner is not None:
                self._ensure(model)
                ops.packnet_view_(p, model.flat_shadow, self.owner, int(k))
        with self._view(model, "PackNet: task_view does not nest", apply, prepare):
            yield model

    # ---- checkpoints between tasks -----------------------------------------------------------------------------------------
    def state_dict(self):
        return {**self._state_tensors(), "task_id": self.task_id, "pruned": self.pruned}

    def load_state_dict(self, sd) -> None:
        self._require_keys(sd, ("task_id", "pruned"))
        self._load_tensors(sd, () if sd["owner"] is None else ("owner", "anchor"))   # (the anchor alone may be None: before the first prune)
        self._pending = False
        self.task_id, self.pruned = int(sd["task_id"]), bool(sd["pruned"])
        self._promise()
