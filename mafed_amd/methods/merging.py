"""Task-vector model merging: task arithmetic (Ilharco et al. 2023), MagMax (Marczak et al. 2024) and TIES (Yadav et al. 2023).

Every task is trained by plain fine-tuning; what is kept of it is its task vector ``tau_t = theta_t - theta_0``, folded at once into a
streaming state laid out like ``model.flat_params`` (memory does not grow with the number of tasks), and the model that is evaluated is
``theta_0 + scaling * merge(tau_1 .. tau_T)``.  The reference ships no implementation, so the arithmetic is this project's (DESIGN.md
section 4p), pinned to the bit: ``tau = fl(theta - base)`` and

    sum      acc = fl(acc + tau)                                          d = acc
    magmax   acc = |tau| > |acc| ? tau : acc   (a tie keeps the earlier)  d = acc
    ties     per tensor: trim the floor((1 - density) m) smallest |tau| (ties at the threshold go with them), then on what is kept
             tau > 0: pos += tau, npos += 1;  tau < 0: neg += tau, nneg += 1
             d = pos / npos where pos + neg > 0,  neg / nneg where pos + neg < 0,  +0.0 otherwise
    apply    p = fl(base + fl(scaling * d)),  shadow = bf16(p)

Nothing runs inside a training step: a run under this plugin is Naive's bit for bit.  ``begin(model)`` captures ``theta_0``, ``update(model)``
folds the task that ended, ``merged_view(model)`` holds the merged model for inference and takes it away again bit for bit, ``merge_(model)``
writes it for good.  Nothing here synchronises with the host but ``trim_report``.  The passes are ``csrc/merge.hip``.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional

import torch

from mafed_amd import ops
from mafed_amd.methods.base import CLStrategy
from mafed_amd.methods.flat import FlatDict, FlatPlugin, behind_optimizer

RULES = ("sum", "magmax", "ties")
MAX_TASKS = 255   # the TIES counters are bytes


class TaskMerging(FlatPlugin, CLStrategy):
    """``TaskMerging(rule="magmax", scaling=1.0, density=0.2, independent=False)``.  ``rule``: ``"sum"`` (task arithmetic), ``"magmax"`` or
    ``"ties"``; ``scaling``: the lambda of the merged model (``merged_view`` and ``merge_`` take another); ``density``: the share of every
    tensor's task vector that TIES keeps, in (0, 1]; ``independent``: every task starts from ``theta_0`` again (``update`` puts it back;
    the optimiser's state stays the caller's business) instead of MagMax's sequential fine-tuning."""
    grads_only_through_model = True    # no hook touches the gradients: Trainer collects the clip norm as it does for Naive
    single_process_only = False        # and nothing of it depends on whose gradients they are
    _WHY_NATIVE = "its passes run on the flat buffers (model.flat_params / model.flat_shadow)"
    _STATE = (("base", torch.float32), ("acc", torch.float32), ("pos", torch.float32), ("neg", torch.float32), ("counts", torch.uint8))

    def __init__(self, rule: str = "magmax", scaling: float = 1.0, density: float = 0.2, independent: bool = False, **kwargs):
        super().__init__(**{k: v for k, v in kwargs.items() if k in ("reg_lambda", "mask", "scaler", "opts")})
        self._check(rule, density)
        self.rule, self.scaling, self.density, self.independent = rule, float(scaling), float(density), bool(independent)
        self.base: Optional[torch.Tensor] = None      # fp32: theta_0
        self.acc: Optional[torch.Tensor] = None       # fp32: the merged delta of sum / magmax
        self.pos: Optional[torch.Tensor] = None       # fp32: TIES, the kept positive mass
        self.neg: Optional[torch.Tensor] = None       #       and the negative one
        self.counts: Optional[torch.Tensor] = None    # uint8 [n, 2]: TIES, the number of tasks in pos and in neg
        self.last_trim_stats: Optional[torch.Tensor] = None   # device int64 [tensors, 4] = {m, r, kept, pattern of the threshold}

    @staticmethod
    def _check(rule, density) -> None:
        if rule not in RULES:
            raise ValueError("TaskMerging: unknown rule %r (one of %s)" % (rule, ", ".join(RULES)))
        if not 0.0 < density <= 1.0:
            raise ValueError("TaskMerging: density must lie in (0, 1], not %r" % (density,))

    # ---- buffers -----------------------------------------------------------------------------------------------------------
    def _ensure(self, model) -> torch.Tensor:
        """The buffers, on the model's device; raises before ``begin`` and for another model."""
        self._native(model)
        if self.base is None:
            raise RuntimeError("TaskMerging: begin(model) has not run (it captures theta_0)")
        return self._place_state(model)

    def named(self, model, which: str = "base") -> FlatDict:
        """name -> view of ``base`` / ``acc`` / ``pos`` / ``neg``, where the rule keeps it."""
        if which == "counts":   # (two to an element: not laid out like the parameters)
            raise KeyError(which)
        return super().named(model, which)

    # ---- between tasks -----------------------------------------------------------------------------------------------------
    def begin(self, model) -> None:
        """Capture ``theta_0``, in front of the first task."""
        p = self._native(model)
        if self.base is not None:
            raise RuntimeError("TaskMerging: begin has run already (theta_0 is captured once)")
        behind_optimizer(model)
        self.base = p.detach().clone()
        if self.rule == "ties":
            self.pos, self.neg = torch.zeros_like(self.base), torch.zeros_like(self.base)
            self.counts = torch.zeros(p.numel(), 2, dtype=torch.uint8, device=p.device)
        else:
            self.acc = torch.zeros_like(self.base)

    def update(self, model, **kwargs) -> None:
        """Fold the task vector of the task that ended."""
        p = self._ensure(model)
        if self._in_view:
            raise RuntimeError("TaskMerging: no update inside a merged_view (the parameters are the merged model, not a task's)")
        if self.rule == "ties" and self.task_id >= MAX_TASKS:
            raise RuntimeError("TaskMerging's TIES counters are bytes: %d tasks at most" % MAX_TASKS)
        behind_optimizer(model)
        if self.rule == "ties":
            # every tensor of the model is a segment; the table and the workspaces are built at the first TIES fold
            segments, (blocks, state, hist) = self._segment_tables(model, list(model._offsets), lambda longest, s: ops.merge_select_blocks(longest))
            drop = 1.0 - self.density
            self.last_trim_stats = ops.merge_ties_fold_(p, self.base, self.pos, self.neg, self.counts, segments, blocks, drop, state=state, hist=hist)
        else:
            ops.merge_fold_(p, self.base, self.acc, self.rule)
        self.task_id += 1
        if self.independent:
            with torch.no_grad():
                p.copy_(self.base)
            model.sync_shadow()

    def trim_report(self, model) -> Dict[str, Dict[str, int]]:
        """name -> {m, r, kept, tau_bits} of the last TIES fold.  The one call of this plugin that synchronises."""
        self._native(model)
        if self.last_trim_stats is None:
            return {}
        rows = self.last_trim_stats.cpu().tolist()
        return {name: dict(zip(("m", "r", "kept", "tau_bits"), row)) for name, row in zip(self._segment_names, rows)}

    # ---- inside a step: nothing --------------------------------------------------------------------------------------------
    def _no_step_in_view(self) -> None:
        if self._in_view:
            raise RuntimeError("TaskMerging: no training step inside a merged_view (the parameters are the merged model)")

    def compute_loss(self, model, loss, **kwargs):
        self._no_step_in_view()
        return loss

    def update_after_backward(self, **kwargs) -> None:
        self._no_step_in_view()

    # ---- the merged model --------------------------------------------------------------------------------------------------
    def _apply(self, model, scaling) -> None:
        p = model.flat_params
        scaling = self.scaling if scaling is None else float(scaling)
        if self.task_id == 0:                         # nothing folded yet: theta_0 itself, bit for bit
            with torch.no_grad():
                p.copy_(self.base)
            model.sync_shadow()
        elif self.rule == "ties":
            ops.merge_apply_(p, model.flat_shadow, self.base, self.pos, "ties", scaling, neg=self.neg, counts=self.counts)
        else:
            ops.merge_apply_(p, model.flat_shadow, self.base, self.acc, self.rule, scaling)

    @contextlib.contextmanager
    def merged_view(self, model, scaling: Optional[float] = None):
        """Inside the block the model is ``theta_0 + scaling * merge(tau_1 .. tau_T)`` (``scaling=None``: the constructor's) for
        ``model(**batch)``, ``generate``, ``sample`` and ``score``.  On exit the parameters and the shadow are put back bit for bit."""
        self._ensure(model)
        with self._view(model, "TaskMerging: merged_view does not nest", lambda: self._apply(model, scaling)):
            yield model

    def merge_(self, model, scaling: Optional[float] = None) -> None:
        """Write the merged model into the parameters and the shadow for good."""
        self._ensure(model)
        if self._in_view:
            raise RuntimeError("TaskMerging: no merge_ inside a merged_view")
        behind_optimizer(model)
        self._apply(model, scaling)

    # ---- checkpoints between tasks -----------------------------------------------------------------------------------------
    def state_dict(self):
        return {**self._state_tensors(), "task_id": self.task_id, "rule": self.rule, "density": self.density}

    def load_state_dict(self, sd) -> None:
        self._require_keys(sd, ("task_id", "rule", "density"))
        self._check(sd["rule"], sd["density"])
        need = ("base", "pos", "neg", "counts") if sd["rule"] == "ties" else ("base", "acc")
        if sd["base"] is not None and any(sd[k] is None for k in need):
            raise ValueError("TaskMerging state of rule %r without %s" % (sd["rule"], [k for k in need if sd[k] is None]))
        self.rule, self.density, self.task_id = sd["rule"], float(sd["density"]), int(sd["task_id"])
        self._load_tensors(sd, need if sd["base"] is not None else ())   # (what the rule does not keep is dropped)
        self.last_trim_stats = None
