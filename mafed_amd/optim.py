"""Optimiser side of the step (reference: mafed/optim/adamw.py, mafed/optim/sched.py,
mafed/model/vqa_cont_learner.py:58-128) on the model's flat parameter / gradient buffers.

``FlatAdamW`` = HF-style AdamW (eps added to sqrt(v) un-corrected, bias correction folded into the step size,
decoupled decay applied after the update with the scheduled lr) as ONE kernel launch per weight-decay segment, with the
global-norm clip scale (Lightning ``gradient_clip_val``, mafed/train.py:288) read from device memory -- the step never
synchronises with the host.  The bf16 shadow weights used by the MFMA GEMMs are written by the same kernel.

``FlatAdam`` / ``FlatAdamax`` = torch.optim.Adam / Adamax (the reference's other two ``optim`` choices, vqa_cont_learner.py:
71-128) on the same buffers: everything but the per-segment update (``_segment_step``) is FlatAdamW's.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from mafed_amd import ops
from mafed_amd.dist import layer_ranges


def lr_lambda(current_step: int, warmup_steps: int, total_steps: int) -> float:
    """get_linear_schedule_with_warmup's multiplier (mafed/optim/sched.py:34-48)."""
    if current_step < warmup_steps:
        return float(current_step) / float(max(1, warmup_steps))
    return max(0.0, float(total_steps - current_step) / float(max(1, total_steps - warmup_steps)))


def compute_warmup(n_batches: int, accumulate_grad_batches: int, warmup_perc: float, warmup_steps: Optional[int] = None) -> Tuple[int, int]:
    """BaseModule.compute_warmup (vqa_cont_learner.py:58-69): the horizon is ceil(len(dl)/accum) * 60 -- the 60 is
    hard-coded upstream -- and warm-up is ``warmup_perc`` of it unless ``warmup_steps`` is configured."""
    total = math.ceil(n_batches / accumulate_grad_batches) * 60
    return total, int(warmup_steps if warmup_steps is not None else warmup_perc * total)


class IncrementalNorm:
    """The global gradient norm in pieces: the backward's gradient hook launches a range's sum-of-squares partials as soon as the range is
    final -- under the rest of the backward -- so that the clip only has the finish kernel left (the one-pass norm reads 1.6 GB on the
    optimiser step's critical path: 0.28 ms at 410M).  Owns the range plan, the partials buffer, the norm log and the record of which
    sweep reported which range."""

    LOG_SLOTS = 4096

    def __init__(self, model):
        """``plan`` = {trigger id: [(lo, hi, first partial slot), ...]} over the flat gradient buffer, in the order the backward finishes
        the ranges (LM head = L, layers L-1 .. 0, embeddings / projector / every bias = -1)."""
        per_layer, head, tail = layer_ranges(model)
        L = len(per_layer)
        trig = {L: [head], -1: list(tail), **{i: [r] for i, r in enumerate(per_layer)}}
        flat = sorted(r for rs in trig.values() for r in rs)
        if not (flat[0][0] == 0 and flat[-1][1] == model.flat_grads.numel() and all(a[1] == b[0] for a, b in zip(flat, flat[1:]))
                and all(lo % 4 == 0 for lo, _ in flat)):
            raise ValueError("the gradient ranges must tile the flat buffer, each from a 16-byte boundary")
        if not all(per_layer[i][0] <= model.layer_matrix_range(i)[0] and model.layer_matrix_range(i)[1] == per_layer[i][1] for i in range(L)):
            raise ValueError("a layer's gradient range must end with its four weight matrices")
        self.model, self.n_layers = model, L
        self.plan, slot = {}, 0
        for t in [L] + list(range(L - 1, -1, -1)) + [-1]:
            self.plan[t] = []
            for lo, hi in trig[t]:
                self.plan[t].append((lo, hi, slot))
                slot += ops.gradnorm_blocks(hi - lo)
        # behind the range partials: 16 slots per layer weight matrix (4 per layer) for the squares the weight-gradient GEMMs' epilogues
        # leave (mafed_gemm_problem.sumsq) -- zero unless a backward uses them (arm)
        self.dw_lo, self.dw_n = slot, 16 * 4 * L
        dev = model.flat_grads.device
        self.partials = torch.zeros(slot + self.dw_n, dtype=torch.float32, device=dev)
        self.log = torch.zeros(self.LOG_SLOTS, dtype=torch.float32, device=dev)   # one slot per fused finish, round robin
        self.log_i = 0
        self.seen: Optional[dict] = None   # {trigger id: serial of the sweep that reported it} since arm(); None = consumed / never armed

    def arm(self, fused_matrix_squares: bool = False):
        """-> hook(i) for ``model.grad_ready_hook``, for the coming backward: called by the sweep on the stream that finished range i.
        ``fused_matrix_squares``: the grouped weight-gradient GEMMs of THIS backward leave the squares of the layers' matrix gradients in
        ``model.dw_sumsq`` slots (their epilogues hold the final values in registers); the hook then reads only a layer's LayerNorm
        weights -- 1.2 GB of the 1.63 GB pass gone.  A sweep that could not fill them says so in its record (then the hook reads the
        whole range)."""
        self.seen = {}
        sq = self.partials[self.dw_lo:]
        sq.zero_()
        self.model.dw_sumsq = sq.view(-1, 4, 16) if fused_matrix_squares else None
        return self.hook

    def hook(self, i) -> None:
        model, sweep = self.model, self.model.last_sweep
        fused = model.dw_sumsq is not None and 0 <= i < self.n_layers and sweep.filled_squares
        for lo, hi, slot in self.plan.get(i, ()):
            if fused:
                hi = model.layer_matrix_range(i)[0]   # the LayerNorm weights in front of the matrices; the matrices' squares are in dw_sumsq
            if hi > lo:
                ops.gradnorm_partial(model.flat_grads[lo:hi], self.partials[slot:])
        if self.seen is None:     # a backward outside Trainer.step() while the hook is still installed (the clip consumed the last
            self.seen = {}        # window's record): its partials are simply never used
        self.seen[i] = sweep.serial
    hook.is_norm_hook = True   # FlatAdamW.arm_norm replaces / removes hooks of this kind only

    def complete(self, serial: int) -> bool:
        """Every range reported during sweep ``serial`` (a sweep that skipped layers, or a plugin's extra sweep after the reports, leaves
        older partials behind: then the buffer is read in one pass)."""
        return self.seen is not None and len(self.seen) == len(self.plan) and all(v == serial for v in self.seen.values())

    def finish(self, max_norm: float, clip_out: torch.Tensor, advance=None, partials: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Fold the partials into ``clip_out`` = {norm, clip scale} -> the norm.  ``advance`` (ops.gradnorm_finish): the schedule advance
        rides in the same launch, and the norm also goes to a log slot of its own, which is what is returned.  ``partials``: somebody
        else's sum-of-squares partials of the whole buffer (``model.final_grad_sumsq``) instead of the hook's."""
        partials = self.partials if partials is None else partials
        if advance is None:
            ops.gradnorm_finish(partials, max_norm, clip_out)
            return clip_out[0]
        i = self.log_i % self.LOG_SLOTS
        self.log_i += 1
        ops.gradnorm_finish(partials, max_norm, clip_out, norm_log=self.log[i:i + 1], advance=advance)
        return self.log[i]


class FlatAdamW:
    """AdamW over ``model.flat_params`` with the reference's two effective parameter groups:
    names without ``bias`` are decayed (LayerNorm weights included), names with ``bias`` are not.
    (The ``vqa_output`` lr_mul groups of configure_optimizers are empty for VLPythia.)"""

    OPTIM = "adamw"
    STATE = ("exp_avg", "exp_avg_sq")   # names of the two per-parameter state buffers (torch's)

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.0,
                 correct_bias: bool = True):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        if not correct_bias:
            raise NotImplementedError("correct_bias=False is not used on the MAFED path")
        self.model = model
        self.base_lr = lr
        self.betas, self.eps, self.weight_decay = tuple(betas), eps, weight_decay
        dev = model.flat_params.device
        for name in self.STATE:
            setattr(self, name, torch.zeros_like(model.flat_params))
        # {lr, 1-b1^t, sqrt(1-b2^t)} of the current step and the step counter live on the DEVICE (mafed_optim_advance):
        # the optimiser kernels carry no per-step host constants, so a whole step replays from a hipGraph
        self.lr_dev = torch.tensor([lr, 1.0, 1.0], dtype=torch.float32, device=dev)
        self.state_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._sched = (0, 0)  # (warmup_steps, total_steps); total 0 = constant lr
        self.clip_out = torch.ones(2, dtype=torch.float32, device=dev)  # {grad norm, clip scale}
        self._clip_pending = False   # clip_grad_norm_ sets, the optimiser pass clears: clip_out holds THIS step's scale (and guards the advance)
        self._advanced = False       # clip_grad_norm_(fuse_advance) sets, advance() clears: the finish launch has advanced the schedule
        # the clip norm from per-range partials that the backward launches; None: the model has no flat layer layout (one-pass norm only)
        self.norm = IncrementalNorm(model) if hasattr(model, "layer_matrix_range") else None
        self.step_count = 0
        n_decay = model.decay_split()
        self.param_groups = [{"lr": lr, "initial_lr": lr, "weight_decay": weight_decay, "range": (0, n_decay)},
                             {"lr": lr, "initial_lr": lr, "weight_decay": 0.0, "range": (n_decay, model.flat_params.numel())}]

    def set_lr(self, lr: float) -> None:
        for g in self.param_groups:
            g["lr"] = lr

    def attach_schedule(self, warmup_steps: int, total_steps: int) -> None:
        """Linear warm-up / decay evaluated on the device each step (get_linear_schedule_with_warmup semantics)."""
        self._sched = (int(warmup_steps), int(total_steps))

    def advance(self) -> None:
        """First kernel of an optimiser step (capturable): t += 1 and {lr(t-1), 1-b1^t, sqrt(1-b2^t)} -> lr_dev.  A no-op when
        clip_grad_norm_(fuse_advance=True) has already done it for this step inside the norm's finish launch."""
        if self._advanced:
            self._advanced = False
            return
        # (with a clip pending the advance is guarded by it: a step whose gradient norm was not finite is skipped on the device --
        #  no parameter / state update in the AdamW kernel, no step-counter advance here; the host sees the non-finite norm in its log)
        ops.optim_advance_(self.state_dev, self.base_lr, self._sched[0], self._sched[1], self.betas[0], self.betas[1], self.lr_dev,
                           clip=self.clip_out if self._clip_pending else None)

    def host_advance(self) -> None:
        """Host mirror of the step counter (logging, state_dict); no device work."""
        self.step_count += 1

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.model.zero_grad()

    # ---- global-norm clip ------------------------------------------------------------------------------------------------
    def begin_incremental_norm(self, fused_matrix_squares: bool = False):
        """-> hook(i) for ``model.grad_ready_hook`` (IncrementalNorm.arm), or None for a model without the flat layer layout."""
        return self.norm.arm(fused_matrix_squares) if self.norm is not None else None

    def arm_norm(self, incremental: bool, fused_matrix_squares: bool = False) -> None:
        """Trainer, in front of every backward of a single process: installs the incremental norm's hook as ``model.grad_ready_hook`` for
        this backward, or removes it.  A hook installed by somebody else is left alone (the norm is then the one-pass form)."""
        if self.norm is None:
            return
        cur = self.model.grad_ready_hook
        if cur is not None and not getattr(cur, "is_norm_hook", False):
            self.norm.seen = None
        elif incremental:
            self.model.grad_ready_hook = self.norm.arm(fused_matrix_squares)
        else:
            self.model.grad_ready_hook = None
            self.model.dw_sumsq = None

    @property
    def advance_fused(self) -> bool:
        """The last clip_grad_norm_(fuse_advance=True) ran the schedule advance in its finish launch: the norm it returned is a log slot of
        its own (stable for IncrementalNorm.LOG_SLOTS steps), and the next advance() launches nothing."""
        return self._advanced

    def clip_grad_norm_(self, max_norm: float, fuse_advance: bool = False) -> torch.Tensor:
        """Global L2 norm + clip scale on the device; the scale is applied inside the AdamW kernel.  Uses the partials handed over in
        ``model.final_grad_sumsq`` if there are any, else those left by the backward's hooks when every range reported in this backward,
        the single pass otherwise.
        ``fuse_advance`` (Trainer): with the partials present, the schedule advance of this optimiser step runs in the finish launch
        (advance() then does nothing) and the returned norm is a view of a log slot of its own -- valid until IncrementalNorm.LOG_SLOTS further
        optimiser steps have run -- instead of ``clip_out[0]``, which the next step overwrites (callers clone that one)."""
        out = self.clip_out[0]
        # sum-of-squares partials of the final gradient, left by whoever wrote it last (A-GEM's projection pass has every element in
        # registers): folded instead of reading the buffer again, and used up.  Every backward sweep drops them at its start.
        handed = getattr(self.model, "final_grad_sumsq", None)
        if handed is not None:
            self.model.final_grad_sumsq = None
        advance = (self.state_dev, self.base_lr, self._sched[0], self._sched[1], self.betas[0], self.betas[1], self.lr_dev) if fuse_advance else None
        if self.norm is not None and (handed is not None or self.norm.complete(self.model.last_sweep.serial)):
            self._advanced = self._advanced or fuse_advance
            out = self.norm.finish(max_norm, self.clip_out, advance=advance, partials=handed)
        elif handed is not None:   # (a model without the flat layer layout: no log slots, no fused advance)
            ops.gradnorm_finish(handed, max_norm, self.clip_out)
        else:
            ops.gradnorm_clip(self.model.flat_grads, max_norm, self.clip_out)
        if self.norm is not None:
            self.norm.seen = None
        self._clip_pending = True
        return out

    def step(self, grad_mul: float = 1.0) -> None:
        self.host_advance()
        self.advance()
        self.apply(grad_mul)

    def apply(self, grad_mul: float = 1.0, zero_grads: bool = False, skip_matrix_zero: bool = False) -> None:
        """Device half of a step: the AdamW kernels, reading this step's scalars from device memory.  ``zero_grads``: the same
        pass also zeroes the gradient buffer (optimizer.zero_grad() of the next window).  ``skip_matrix_zero`` (with ``zero_grads``): the
        layers' weight-matrix gradients are left as they are -- the next window's first backward overwrites them (model.grad_overwrite);
        the pass then runs chunk by chunk (``_chunks()``), otherwise as one launch per weight-decay segment."""
        if zero_grads and skip_matrix_zero:
            self._pass(self._chunks(), grad_mul, True, skip_matrix_zero=True)
        else:
            self._pass([(None, *g["range"], g["weight_decay"]) for g in self.param_groups if g["range"][1] > g["range"][0]], grad_mul, zero_grads)

    def _segment_step(self, lo: int, hi: int, wd: float, clip, grad_mul: float, zero_grad: bool, zero_n: Optional[int] = None) -> None:
        """The update rule on flat range [lo, hi) with weight decay ``wd``: one launch, the bf16 shadow written and (``zero_grad``) the
        gradient zeroed in the same pass -- all of it, or only its first ``zero_n`` elements."""
        m = self.model
        shadow = m.flat_shadow[lo:hi] if m.flat_shadow is not None else None
        ops.adamw_step_(m.flat_params[lo:hi], m.flat_grads[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], self.lr_dev,
                        self.betas[0], self.betas[1], self.eps, wd, 0, clip, grad_mul, shadow, zero_grad=zero_grad, zero_n=zero_n)

    def _pass(self, chunks, grad_mul: float, zero_grads: bool, skip_matrix_zero: bool = False, events: Optional[dict] = None, stream=None) -> None:
        """One optimiser pass on the current stream: one launch per (key, lo, hi, weight_decay) of ``chunks``, the gradient zeroed in the same
        pass if ``zero_grads`` -- of a layer chunk only its LayerNorm-weight part when ``skip_matrix_zero`` (mafed_adamw_step_partial_zero) --,
        an event of ``stream`` per chunk into ``events``; then the end of the pass: the clip scale is used up, the bf16 shadow is current."""
        m = self.model
        clip = self.clip_out if self._clip_pending else None
        for key, lo, hi, wd in chunks:
            zn = None
            if skip_matrix_zero and isinstance(key, tuple) and key[0] == "layer":
                mlo, mhi = m.layer_matrix_range(key[1])
                assert lo <= mlo and mhi == hi, "layer chunk = [LayerNorm weights | weight matrices]"
                zn = mlo - lo
            self._segment_step(lo, hi, wd, clip, grad_mul, zero_grad=zero_grads, zero_n=zn)
            if events is not None:
                events[key] = stream.record_event()
        if skip_matrix_zero:
            m._dw_stale = True   # (cleared by the next backward sweep: it overwrites the matrices, or zeroes them first)
        self._clip_pending = False
        if m.flat_shadow is not None:
            m._shadow_dirty = False

    def _chunks(self):
        """(key, lo, hi, weight_decay) in the order the NEXT forward touches the parameters: everything the first kernels
        read (all biases / non-decayed tensors, token embedding, projector), then the layers bottom-up, then final LN + head."""
        m = self.model
        wd = self.param_groups[0]["weight_decay"]
        per_layer, head, tail = layer_ranges(m)
        out = [("pre", tail[-1][0], tail[-1][1], 0.0)]               # the non-decayed segment
        out += [("pre", lo, hi, wd) for lo, hi in tail[:-1]]          # embed_in, projector
        out += [(("layer", i), lo, hi, wd) for i, (lo, hi) in enumerate(per_layer)]
        out.append(("head", head[0], head[1], wd))
        assert sum(hi - lo for _, lo, hi, _ in out) == m.flat_params.numel(), "optimizer chunks must tile the flat buffer"
        return [c for c in out if c[2] > c[1]]

    def apply_pipelined(self, stream, grad_mul: float = 1.0, zero_grads: bool = True, skip_matrix_zero: bool = False):
        """AdamW (and the gradient zeroing) chunk by chunk on ``stream``, one event per chunk group: the next forward waits
        for "pre", then for ("layer", i) right before layer i, then for "head" -- so the HBM-bound update of the upper layers
        runs under the MFMA-bound forward of the lower ones instead of in front of it.  The caller's stream must not touch
        parameters, optimiser state or gradients until it has waited for these events (the model's forward does)."""
        main = torch.cuda.current_stream()
        stream.wait_event(main.record_event())  # gradients final, clip scale and {lr, bias corrections} on the device
        events = {}
        with torch.cuda.stream(stream):
            self._pass(self._chunks(), grad_mul, zero_grads, skip_matrix_zero=zero_grads and skip_matrix_zero, events=events, stream=stream)
        return events

    def state_dict(self):
        sd = {name: getattr(self, name) for name in self.STATE}
        sd.update({"optim": self.OPTIM, "step": self.step_count, "sched": self._sched})
        return sd

    def load_state_dict(self, sd):
        # (a dict without "optim" predates the other rules: it is AdamW's)
        other = sd.get("optim", "adamw")
        if other != self.OPTIM or any(name not in sd for name in self.STATE):
            raise ValueError("%s cannot load the state of optimiser %r (keys %s)" % (type(self).__name__, other, sorted(sd)))
        for name in self.STATE:
            getattr(self, name).copy_(sd[name])
        self.step_count = int(sd["step"])
        self.state_dev.fill_(self.step_count)
        self._sched = tuple(sd.get("sched", self._sched))


class _FlatTorchAdam(FlatAdamW):
    """torch.optim.Adam-family rules on FlatAdamW's machinery (segments, device schedule, clip, chunked / pipelined passes): only the
    per-segment update differs -- one mafed_adam_step / mafed_adamax_step launch."""

    _RULE = ""

    def __init__(self, model, lr: float, betas, eps: float, weight_decay: float):
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

    def _segment_step(self, lo: int, hi: int, wd: float, clip, grad_mul: float, zero_grad: bool, zero_n: Optional[int] = None) -> None:
        m = self.model
        shadow = m.flat_shadow[lo:hi] if m.flat_shadow is not None else None
        zn = 0 if not zero_grad else (hi - lo if zero_n is None else min(int(zero_n), hi - lo))
        ops.adam_family_step_(self._RULE, m.flat_params[lo:hi], m.flat_grads[lo:hi], self.exp_avg[lo:hi], getattr(self, self.STATE[1])[lo:hi],
                              self.lr_dev, self.betas[0], self.betas[1], self.eps, wd, 0, clip, grad_mul, shadow, zero_n=zn)


class FlatAdam(_FlatTorchAdam):
    """torch.optim.Adam (torch 2.x single-tensor rule; config.optim = "adam") over the two weight-decay segments: the decay is
    coupled (L2, added to the gradient) and eps comes after the bias correction.  Defaults are torch's."""

    OPTIM = _RULE = "adam"
    STATE = ("exp_avg", "exp_avg_sq")

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class FlatAdamax(_FlatTorchAdam):
    """torch.optim.Adamax (config.optim = "adamax"): g' and m as for Adam, u = max(b2*u, |g'| + eps) in ``exp_inf``,
    p -= lr/(1-b1^t) * m/u.  Defaults are torch's."""

    OPTIM = _RULE = "adamax"
    STATE = ("exp_avg", "exp_inf")

    def __init__(self, model, lr: float = 2e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class LinearWarmupSchedule:
    """LambdaLR(get_linear_schedule_with_warmup) equivalent for FlatAdamW: lr is set at construction (epoch 0) and
    after every ``step()``."""

    def __init__(self, optimizer: FlatAdamW, warmup_steps: int, total_steps: int, last_epoch: int = -1):
        self.optimizer, self.warmup_steps, self.total_steps = optimizer, warmup_steps, total_steps
        self.last_epoch = last_epoch
        optimizer.attach_schedule(warmup_steps, total_steps)  # the device evaluates the same lambda from its own step counter
        self.step()

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def step(self) -> None:
        """Host mirror (param_groups[...]["lr"], get_last_lr); the kernels read the device-side value."""
        self.last_epoch += 1
        self.optimizer.set_lr(self.optimizer.base_lr * lr_lambda(self.last_epoch, self.warmup_steps, self.total_steps))


def get_linear_schedule_with_warmup(optimizer: FlatAdamW, warmup_steps: int, total_steps: int, last_epoch: int = -1) -> LinearWarmupSchedule:
    return LinearWarmupSchedule(optimizer, warmup_steps, total_steps, last_epoch)
