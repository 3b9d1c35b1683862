"""MAFED -- feature distillation with separate vision / language weights (reference: mafed/methods/distillation.py).

Same constructor kwargs and method names as the reference plugin.  The per-layer, per-modality arithmetic runs in
the fused dual-mask kernels (``mafed_distill_fwd/bwd``): one pass over a layer's student/teacher hidden states
yields both modality sums; all layers go through ONE autograd node, the scalar algebra (counts, modality weights,
layer coefficients) is vectorised over layers on the device, and nothing synchronises with the host (the
reference's per-layer ``wandb.log(.item())``, distillation.py:165, becomes ``self.last_layer_losses``).
"""
from __future__ import annotations

from copy import deepcopy
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from mafed_amd import ops
from mafed_amd.methods.base import CLStrategy
from mafed_amd.methods.distillation_loss_weights import DistillationWeights
from mafed_amd.methods.flat import require_native
from mafed_amd.methods.memory import HBMReplayBuffer, dataset_len, take_samples
from mafed_amd.methods.replay import make_memory_selection, select_memory_indices


import os as _os
_EARLY_SUMS = _os.environ.get("MAFED_EARLY_SUMS", "1") == "1"


class _DistillSumsFn(torch.autograd.Function):
    """sums[l] = {sum_lang d, sum_vision d, n_lang, n_vision} for every distilled layer l (d = per-token MSE or 1-cos)."""

    @staticmethod
    def forward(ctx, attention_mask, P, cosine, teacher: Sequence[torch.Tensor], *student):
        nl = len(student)
        out = torch.empty((nl, 4), dtype=torch.float32, device=student[0].device)
        for l in range(nl):
            ops.distill_fwd(student[l], teacher[l], attention_mask, P, cosine, out=out[l])
        ctx.am, ctx.P, ctx.cosine, ctx.teacher = attention_mask, P, cosine, list(teacher)
        ctx.save_for_backward(*student)
        return out

    @staticmethod
    def backward(ctx, g):
        student = ctx.saved_tensors
        g = g.contiguous()
        grads = []
        for l, s in enumerate(student):
            if ctx.needs_input_grad[4 + l]:
                grads.append(ops.distill_bwd(s, ctx.teacher[l], ctx.am, ctx.P, g[l], ctx.cosine))
            else:
                grads.append(None)
        return (None, None, None, None, *grads)


def global_token_counts(sums: torch.Tensor, group=None) -> torch.Tensor:
    """SURVEY.md section 8e, the optional exact normaliser: under data parallelism every rank divides its masked sums by ITS OWN
    token counts (mafed/methods/distillation.py:248, distillation_loss_weights.py:148-155 see the local batch), so the gradient mean
    over ranks weights ranks with fewer valid text tokens more.  Replacing {n_lang, n_vision} by their mean over ranks (one all-reduce
    of two floats per layer row) makes  mean_ranks(loss_r)  equal the loss of ONE process holding the concatenated batch:
    sum_r S_r / sum_r n_r.  Returns a new [nl, 4] tensor; identity without an initialised multi-rank group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) < 2:
        return sums
    out = sums.clone()
    counts = out[:, 2:4].contiguous()
    dist.all_reduce(counts, group=group)
    out[:, 2:4] = counts / dist.get_world_size(group)
    return out


_ZERO_SCALARS: Dict[str, torch.Tensor] = {}


def _zero_scalar(device) -> torch.Tensor:
    z = _ZERO_SCALARS.get(str(device))
    if z is None:
        z = _ZERO_SCALARS[str(device)] = torch.zeros((), device=device)
    return z


class _FusedDistillLossFn(torch.autograd.Function):
    """The whole MSE distillation term of the native model as ONE node: the per-layer masked sums (started layer by layer
    during the student forward, or computed here), then ``mafed_distill_combine`` -- masked means, modality weights, layer
    coefficients and the scalar loss in one launch (the reference's per-layer Python loop, distillation.py:109-120, as ~12
    torch kernels per step before).  The backward materialises nothing: it leaves d loss / d sums (one device row per layer,
    scaled by the upstream gradient) in the model's activation record, and the model's own backward adds
    coef * 2/h * (x - teacher) to the residual-stream gradient inside the LayerNorm-backward kernel of that layer
    (mafed_layernorm_bwd, teacher != NULL) -- no per-layer gradient tensor, no separate add / cast pass.
    Outputs: (loss, per_layer [nl], modality [nl, 2]); only the loss is differentiable."""

    @staticmethod
    def forward(ctx, hook, attention_mask, P, teacher: Sequence[torch.Tensor], sv, layers, early, coeffs, mode, lang_w, lang_vec, cosine, exact_group, *student):
        nl = len(student)
        if early is not None:
            # the sums were started layer by layer during the student forward (FeatureDistillation._early_sums_hook)
            sums, ev = early
            torch.cuda.current_stream().wait_event(ev)
        else:
            sums = torch.empty((nl, 4), dtype=torch.float32, device=student[0].device)
            for l in range(nl):
                ops.distill_fwd(student[l], teacher[l], attention_mask, P, bool(cosine), out=sums[l])
        if exact_group is not None:
            sums = global_token_counts(sums, exact_group)
        loss, per_layer, modality, inject = ops.distill_combine(sums, coeffs, mode, lang_w, lang_vec)
        ctx.sv, ctx.layers, ctx.teacher, ctx.inject, ctx.cosine = sv, list(layers), list(teacher), inject, bool(cosine)
        ctx.mark_non_differentiable(per_layer, modality)
        return loss.reshape(()), per_layer, modality

    @staticmethod
    def backward(ctx, g, _gp, _gm):
        scaled = ctx.inject * g  # [nl, 4] x upstream d / d loss (1 / accumulate_grad_batches under the Trainer)
        ctx.sv["inject"] = {layer: (ctx.teacher[k], scaled[k]) for k, layer in enumerate(ctx.layers)}
        ctx.sv["inject_cosine"] = ctx.cosine
        ctx.sv = None
        # (the hook's "gradient" only makes the model's node run; its value is never read: a cached zero scalar -- no fill kernel per
        #  step, and nothing uninitialised for anomaly detection or an accidental accumulation to pick up)
        return (_zero_scalar(g.device),) + (None,) * (12 + len(ctx.layers))


class _DistillClsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, t):
        ctx.save_for_backward(s)
        ctx.teacher = t    # a detached tensor or ops.TeacherRows (rows of the teacher cache, read in place)
        return ops.distill_cls_fwd(s, t).reshape(())

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        coef = (g.reshape(1) / s.shape[0]).contiguous()
        return ops.distill_cls_bwd(s, ctx.teacher, coef), None


def _cache_dtype(dtype) -> torch.dtype:
    """``teacher_cache_dtype``: torch.float32 / "fp32" or torch.bfloat16 / "bf16"."""
    named = {"fp32": torch.float32, "bf16": torch.bfloat16}
    if isinstance(dtype, str) and dtype in named:
        return named[dtype]
    if dtype in (torch.float32, torch.bfloat16):
        return dtype
    raise ValueError(f"teacher_cache_dtype must be torch.float32 / 'fp32' or torch.bfloat16 / 'bf16', not {dtype!r}")


class FeatureDistillation(CLStrategy):
    """Feature Distillation with Separate Vision & Language Weights (MAFED)."""
    grads_only_through_model = True  # every parameter gradient of a step comes out of the model's own backward (Trainer: incremental clip norm)

    def __init__(self, memory_size, opts, model_type, distillation_modality_weighing_strategy="equal",
                 distillation_layer_weighing_strategy="single", distillation_coeff=1.0, replay_coeff=1.0,
                 distillation_layer=-1, cls_distillation=False, distillation_loss="mse", gamma: float = 0.8,
                 num_hidden_layers: int = 11, memory_selection=None, **kwargs):
        super().__init__(opts=opts, **{k: v for k, v in kwargs.items() if k in ("reg_lambda", "mask", "scaler")})
        self.memory_size = memory_size
        num_mem_tasks = len(opts.tasks) - 1
        self.memory_per_task = int(memory_size / num_mem_tasks)
        self.batch_size = opts.batch_size
        self.num_workers = getattr(opts, "n_workers", 0)
        self.seed = 1
        self.datasets: List = []
        self.rng = np.random.default_rng(opts.seed)  # memory sub-sampling stream, as upstream (distillation.py:45)
        # None: that random subset.  "herding" / "kcenter" / a MemorySelection: chosen in the new teacher's pooled feature space
        self.memory_selection = make_memory_selection(memory_selection)
        self.pin_mem = getattr(opts, "pin_mem", False)
        self.step = 0
        self.model_type = model_type
        self.past_model = None
        self.replay_coeff = replay_coeff
        self.distillation_coeff = distillation_coeff
        self.weighing_strategy = distillation_modality_weighing_strategy
        self._cls_distillation = cls_distillation
        self._cosine = distillation_loss == "cosine"
        # a layer outside [0, num_hidden_layers) means "no single layer" (distillation.py:61-64)
        layer = distillation_layer if (distillation_layer is not None and 0 <= distillation_layer < num_hidden_layers) else None
        self.loss_weights = DistillationWeights(
            distillation_modality_weighing_strategy=distillation_modality_weighing_strategy,
            distillation_layer_weighing_strategy=distillation_layer_weighing_strategy, gamma=gamma,
            num_hidden_layers=num_hidden_layers, distillation_layer=layer)
        self.opts = opts
        self.num_vision_tokens = 256  # hard-coded upstream (distillation.py:73); instance attribute, settable
        self.mem_dataloader = None
        self.overlap_teacher = True
        self.fused_distill = True  # distillation gradient (MSE or cosine) injected inside the model's LayerNorm-backward kernels
        # data parallel only: masked means over the GLOBAL token counts (one small all-reduce per step; global_token_counts).  Off = the
        # reference's per-rank means.  True = default process group, or pass a group.
        self.exact_normaliser = kwargs.get("exact_normaliser", False)
        # keep the frozen teacher's distilled hidden states for the whole replay memory resident in HBM (build_teacher_cache; filled by
        # update() once per task).  Off by default: the reference runs the teacher forward in every replay step.
        self.teacher_cache = bool(kwargs.get("teacher_cache", False))
        # storage type of that cache.  fp32 (default) keeps the step bit-identical to the per-step teacher forward.  bf16 halves the
        # memory and the traffic but CHANGES THE TARGET: every teacher element is rounded to 8 significant bits (relative error <= 2^-9)
        # and the student is pulled towards the rounded teacher.
        self.teacher_cache_dtype = _cache_dtype(kwargs.get("teacher_cache_dtype", torch.float32))
        self._tcache = None
        self._mem_index = None
        self._prefetched = None
        self.last_layer_losses: Optional[torch.Tensor] = None  # [n_layers] device tensor of the last distill() call
        self.last_modality_losses: Optional[torch.Tensor] = None  # [n_layers, 2] (lang, vision)

    # ---- between tasks -----------------------------------------------------------------------------------------------
    def update(self, dataset, model, dataloader, mask=None, **kwargs):
        if self.memory_selection is not None:   # (raises before the teacher is replaced)
            if model is None:
                raise ValueError("FeatureDistillation: memory_selection needs the model that finished the task")
            require_native(model, "FeatureDistillation", "memory_selection reads its pooled hidden states (model.pooled_features)")
        self._update_model(model)
        self._update_memory(dataset)
        self.loss_weights.update_weights(model, dataloader, self.task_id)
        self.task_id += 1
        if getattr(self, "teacher_cache", False):   # opt-in: the new teacher's states for the whole memory, once per task
            self.build_teacher_cache()

    def _update_model(self, model):
        """Teacher := frozen copy of the finished task's model (distillation.py:211-213)."""
        self.drop_teacher_cache()   # states of the previous teacher
        self.past_model = deepcopy(model)
        self.past_model.eval()
        for p in self.past_model.parameters():
            p.requires_grad_(False)

    def _update_memory(self, dataset):
        """Keep ``memory_per_task`` samples of the finished task: a random subset (distillation.py:182-209), or with ``memory_selection``
        set the ones it picks in the new teacher's feature space.

        ``dataset`` may be (a) an ``HBMReplayBuffer``-compatible dict of collated tensors, (b) any map-style dataset
        whose items are dicts of tensors of equal text length (collated with torch.stack)."""
        n = dataset_len(dataset)
        k = min(self.memory_per_task, n)
        if self.memory_selection is None:
            idx = self.rng.choice(np.arange(n), k, replace=False)
        else:
            idx = select_memory_indices(self.memory_selection, self.past_model, dataset, k, "FeatureDistillation")
        assert len(set(idx.tolist())) == k
        self.seed = 1
        samples = take_samples(dataset, idx, HBMReplayBuffer.KEYS)
        self.datasets.append(samples)
        if not isinstance(self.mem_dataloader, HBMReplayBuffer):
            import torch.distributed as dist
            rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
            dev = self.past_model.flat_params.device if hasattr(self.past_model, "flat_params") else samples["input_ids"].device
            self.mem_dataloader = HBMReplayBuffer(self.batch_size, dev, seed=self.opts.seed, rank=rank, world_size=world)
        self.mem_dataloader.add(samples)

    def update_mask(self, mask=None):
        return None

    def update_after_new_task(self, model, dataset):
        if self.weighing_strategy != "loss_based":  # never true upstream either (distillation.py:168-173)
            return
        raise NotImplementedError("loss_based weighing does not exist in the reference code path")

    def update_after_step(self, model, batch_idx=0, on_train_start=False):
        if self.task_id == 0 or self.weighing_strategy != "dynamic":
            return
        raise NotImplementedError("dynamic weighing does not exist in the reference code path")

    # ---- inside a step ---------------------------------------------------------------------------------------------------
    def compute_loss(self, model, loss, batch=None, **kwargs):
        return loss

    def replay(self, model):
        """Memory batch -> replay CE (iff replay_coeff > 0 and task_id > 0) + distillation (distillation.py:84-103)."""
        batch = next(iter(self.mem_dataloader))
        self._mem_index = batch.pop("memory_index", None)   # (HBMReplayBuffer.attach_index: rows of the teacher cache)
        n_ex = batch["input_ids"].size(0)
        do_replay = self.replay_coeff > 0 and self.task_id > 0
        pv = batch.get("pixel_values")
        ready = getattr(self.mem_dataloader, "last_ready_event", None)
        if "patch_embeddings" not in batch and torch.is_tensor(pv) and pv.dim() == 4 and hasattr(model, "get_patch_embeddings"):
            # images in the memory batch: ONE pass through the frozen tower serves student and teacher (upstream encodes the
            # same images twice per step, distillation.py:91 and :222 -- the teacher's deep-copied tower holds the same weights)
            with torch.no_grad():
                batch["patch_embeddings"] = model.get_patch_embeddings(pv)
            # the features were just written on THIS stream: the loader's event says nothing about them, the teacher's stream has
            # to wait for everything queued here (an event recorded after the tower), not for the loader
            ready = None
        # ``run``: the batch at the text length the engine runs it at (the model's text_bucket; ``batch`` itself when nothing is appended).
        # Student, teacher and the distillation kernels all see ``run``; the caller's dict keeps its shapes.
        run, ready = self._engine_batch(model, batch, ready)
        if self.distillation_coeff != 0:
            # frozen-teacher forward on a second HIP stream, concurrent with the student's
            self._prefetch_teacher(run, ready)
        hooked = self._install_early_sums(model, run)
        try:
            output = model(**run, compute_loss=do_replay, output_hidden_states=True, return_dict=True)
        finally:
            if hooked:
                model.hidden_ready_hook = None
        # (x * 1.0 is x: with the default coefficient the product and its backward are two scalar kernels on the stream between the
        # forward and the backward for nothing)
        loss = (output.loss if self.replay_coeff == 1.0 else self.replay_coeff * output.loss) if do_replay else None
        if self.distillation_coeff == 0:
            return loss, n_ex
        dloss = self.distill(output=output, batch=batch, run=run)
        loss = dloss if loss is None else loss + dloss
        return loss, n_ex

    def _engine_batch(self, model, batch, ready=None):
        """(the batch right-padded to the model's bucketed text length, the event its tensors are ready at).  One launch for ids, mask and
        labels; with a loader that hands out an event it runs on the teacher's stream, so that the teacher forward still starts behind the
        loader alone and not behind the caller's stream (_prefetch_teacher)."""
        if not hasattr(model, "padded_text_len"):
            return batch, ready
        B, T = batch["input_ids"].shape
        if model.padded_text_len(B, T) == T:
            return batch, ready
        pm = self.past_model
        parts = (batch["input_ids"], batch["attention_mask"], batch.get("labels"))
        if (ready is not None and self.distillation_coeff != 0 and self.overlap_teacher and hasattr(pm, "side_stream") and pm.flat_params.is_cuda):
            main, side = torch.cuda.current_stream(), pm.side_stream()
            side.wait_event(ready)
            with torch.cuda.stream(side):
                padded = model.pad_text_batch(*parts)
                ready = side.record_event()
            for src, dst in zip(parts, padded):
                if src is not None and src.is_cuda:
                    src.record_stream(side)
                if dst is not None:
                    dst.record_stream(main)
            main.wait_event(ready)
        else:
            padded = model.pad_text_batch(*parts)
            ready = None   # written on this stream: the teacher's stream waits for it, not for the loader
        run = dict(batch)
        run["input_ids"], run["attention_mask"] = padded[0], padded[1]
        if padded[2] is not None:
            run["labels"] = padded[2]
        return run, ready

    def _cached(self, key, make):
        """Constant device tensors of the step (mask pieces, the coefficient vector), built once per shape instead of per step."""
        cache = self.__dict__.setdefault("_const_cache", {})
        v = cache.get(key)
        if v is None:
            v = cache[key] = make()
        return v

    def _install_early_sums(self, model, batch) -> bool:
        """Fused MSE path only: start each distilled layer's masked sums (one HBM-bound pass over student + teacher states)
        as soon as the student forward has produced that hidden state, on the teacher's stream, instead of running all of
        them back to back after the forward -- they then run under the following layers' GEMMs."""
        self._early = None
        pre = getattr(self, "_prefetched", None)
        if (not _EARLY_SUMS or pre is None or self._cls_distillation or not self.fused_distill or not self.overlap_teacher
                or not hasattr(model, "hidden_ready_hook") or not torch.is_grad_enabled()):
            return False
        hs, ev, n = pre
        layers = list(self.loss_weights.get_distillation_layers())
        if not layers or max(layers) + 1 > n:
            return False
        dev = batch["attention_mask"].device if batch["attention_mask"].is_cuda else self.past_model.flat_params.device
        am = batch["attention_mask"].to(dev, torch.int64).contiguous()
        P = self.num_vision_tokens
        B, T = am.shape
        side = self.past_model.side_stream()
        sums = torch.empty((len(layers), 4), dtype=torch.float32, device=dev)
        slot = {l: k for k, l in enumerate(layers)}
        state = {"sums": sums, "stream": side, "layers": layers, "n": len(layers)}
        cosine = bool(self._cosine)

        def hook(l, x):
            k = slot.get(l)
            if k is None:
                return
            main = torch.cuda.current_stream()
            side.wait_event(main.record_event())   # hidden_states[l] is final on the caller's stream
            with torch.cuda.stream(side):           # (the teacher forward that produced hs[l] ran on this very stream)
                ops.distill_fwd(x.view(B, P + T, -1), hs[l], am, P, cosine, out=sums[k])

        model.hidden_ready_hook = hook
        self._early = state
        return True

    def _prefetch_teacher(self, batch, batch_ready_event=None):
        """Issue the teacher forward on its own stream before the student's (same arithmetic, earlier in time): the two
        forwards are independent kernel chains, so their wave-quantisation tails fill each other on the 256 CUs."""
        self._prefetched = None
        pm = self.past_model
        if not (self.overlap_teacher and hasattr(pm, "hidden_states_upto") and pm.flat_params.is_cuda):
            return
        layers = self.loss_weights.get_distillation_layers()
        main = torch.cuda.current_stream()
        side = pm.side_stream()
        # Order behind the previous step's backward (the last reader of the previous teacher states, whose memory this
        # forward re-uses) ...
        ev_prev = getattr(self, "backward_done_event", None)
        if ev_prev is not None:
            side.wait_event(ev_prev)
        # ... and behind whatever produced this batch.  A loader that gathers on its own stream (HBMReplayBuffer) hands
        # out the batch's event: the teacher forward then does NOT wait for the caller's stream, i.e. it overlaps the
        # HBM-bound clip + AdamW tail of the previous step (the frozen teacher does not depend on the update).
        # Otherwise: everything queued on the caller's stream so far.
        side.wait_event(batch_ready_event if batch_ready_event is not None else main.record_event())
        for v in batch.values():
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(side)
        kw = {"patch_embeddings": batch["patch_embeddings"]} if "patch_embeddings" in batch else {"pixel_values": batch["pixel_values"]}
        with torch.cuda.stream(side):
            # teacher cache: its rows, read in place, instead of the forward
            hs = self._teacher_rows(max(layers) + 1, consumer=main, S=self.num_vision_tokens + batch["input_ids"].shape[1])
            if hs is None:
                hs = [x.detach() for x in pm.hidden_states_upto(batch["input_ids"], batch["attention_mask"], n_hidden=max(layers) + 1, **kw)]
            ev = side.record_event()
        self._prefetched = (hs, ev, max(layers) + 1)

    def _get_past_hidden_states(self, batch, n_hidden: Optional[int] = None, run=None):
        """Frozen-teacher hidden states; pops ``labels`` from the caller's dict like upstream (distillation.py:218-224).  ``run``: the batch
        as the engine runs it (_engine_batch), when that is not ``batch``."""
        batch.pop("labels", None)
        if run is not None and run is not batch:
            batch = {k: v for k, v in run.items() if k != "labels"}
        pre = getattr(self, "_prefetched", None)
        if pre is not None:
            self._prefetched = None
            hs, ev, n = pre
            if n_hidden is None or n >= n_hidden:
                torch.cuda.current_stream().wait_event(ev)
                return hs
        pm = self.past_model
        with torch.no_grad():
            cached = self._teacher_rows(n_hidden, S=self.num_vision_tokens + batch["input_ids"].shape[1])
            if cached is not None:
                return cached
            if hasattr(pm, "hidden_states_upto"):
                kw = {"patch_embeddings": batch["patch_embeddings"]} if "patch_embeddings" in batch else {"pixel_values": batch["pixel_values"]}
                return [x.detach() for x in pm.hidden_states_upto(batch["input_ids"], batch["attention_mask"], n_hidden=n_hidden, **kw)]
            hs = pm(**batch, output_hidden_states=True, return_dict=True).hidden_states
            return [x.detach() for x in hs]

    # ---- teacher cache (MI355X-only design point: 288 GB of HBM) ------------------------------------------------------------
    def build_teacher_cache(self, mem=None, batch_size: Optional[int] = None, dtype=None) -> Dict[str, float]:
        """The frozen teacher sees the same stored samples for a whole task: run it ONCE over (this rank's shard of) the replay
        memory and keep the distilled hidden states resident -- [n_layers, n, S, h]; in fp32 27 MB per sample at 410M = 108 GB for the
        reference's 4000-sample memory, sharded 1/N under data parallelism.  A replay step then skips the teacher forward (5.2 of the
        step's 22.5 TFLOP): its distillation kernels read the batch's rows where they are stored, through the buffer's
        ``memory_index`` (``ops.TeacherRows``) -- no gathered copy.  The cache is written by the same kernels on the same batch shapes
        as the per-step forward (the tail re-runs the last full batch), so the fp32-cached step is bit-identical to the uncached one.
        ``dtype`` (default: ``self.teacher_cache_dtype``) torch.bfloat16 / "bf16" stores the states rounded to nearest even, half the
        size; the step then distils towards the ROUNDED teacher (relative rounding <= 2^-9 per element), not a bit-identical one.
        Dropped whenever the teacher changes (``_update_model``)."""
        import time
        dtype = _cache_dtype(dtype if dtype is not None else getattr(self, "teacher_cache_dtype", torch.float32))
        mem = mem if mem is not None else self.mem_dataloader
        pm = self.past_model
        if pm is None or not hasattr(pm, "hidden_states_upto") or not hasattr(mem, "data") or len(mem) == 0:
            raise RuntimeError("teacher cache: needs the native teacher and a resident replay memory (HBMReplayBuffer)")
        if mem.data.get("patch_embeddings") is None:
            raise RuntimeError("teacher cache: the replay memory must hold pre-encoded ``patch_embeddings`` (it stores ``pixel_values``: "
                               "encode them once with model.get_patch_embeddings before adding the samples)")
        layers = list(self.loss_weights.get_distillation_layers())
        n_hidden = max(layers) + 1
        lo, hi = mem.shard() if hasattr(mem, "shard") else (0, len(mem))
        B = int(batch_size or mem.batch_size)
        data = mem.data
        dev = pm.flat_params.device
        T = data["input_ids"].shape[1]
        n = hi - lo
        # rows are stored at the length the forward that fills them runs at: the teacher's text_bucket applied to the batches below (all of
        # min(B, n) samples), i.e. what a replay step of the same batch size reads
        Tp = pm.padded_text_len(min(B, n), T) if hasattr(pm, "padded_text_len") and n > 0 else T
        S, h = self.num_vision_tokens + Tp, pm.config.hidden_size
        if n <= 0:
            raise RuntimeError(f"teacher cache: this rank's shard of the replay memory is empty ({len(mem)} samples over the ranks)")
        t0 = time.time()
        states = torch.empty((len(layers), n, S, h), dtype=dtype, device=dev)
        with torch.no_grad():
            for i in range(lo, hi, B):
                j = min(i, max(lo, hi - B))            # the tail re-runs the last FULL batch: same kernel shapes as in the step
                e = min(j + B, hi)
                ids, am = data["input_ids"][j:e], data["attention_mask"][j:e]
                if Tp != T:
                    ids, am, _ = pm.pad_text_batch(ids, am)   # (fed at the padded length, the forward hands its states out untrimmed)
                hs = pm.hidden_states_upto(ids, am, patch_embeddings=data["patch_embeddings"][j:e], n_hidden=n_hidden)
                if hs[0].shape[1] != S:
                    raise RuntimeError(f"teacher cache: the forward ran at {hs[0].shape[1]} positions, the cache was sized for {S}")
                for k, l in enumerate(layers):
                    if dtype == torch.float32:
                        states[k, j - lo: e - lo] = hs[l].view(e - j, S, h)
                    else:
                        ops.cast(hs[l].contiguous().view(e - j, S, h), dtype, out=states[k, j - lo: e - lo])   # round to nearest even
        torch.cuda.synchronize(dev)
        mem.attach_index = True
        mem._next = None      # (a batch gathered ahead carries no index)
        self._tcache = {"states": states, "layers": layers, "lo": lo, "n": n, "S": S, "T": T, "h": h, "mem": mem, "mem_len": len(mem), "streams": set(),
                        "layer_off": (torch.arange(len(layers), device=dev, dtype=torch.int64) * (n * S)).view(-1, 1, 1),
                        "ar": torch.arange(S, device=dev, dtype=torch.int64).view(1, 1, S)}
        return {"GB": states.numel() * states.element_size() / 1e9, "samples": n, "seconds": time.time() - t0}

    def drop_teacher_cache(self) -> None:
        tc = getattr(self, "_tcache", None)
        if tc is not None and hasattr(tc["mem"], "attach_index"):
            tc["mem"].attach_index = False
            tc["mem"]._next = None
        self._tcache = None

    def _cache_for_batch(self, S: Optional[int] = None):
        """(cache, memory index of the batch handed out last, distilled layers), or None when the cache does not cover that batch.
        ``S``: the positions per sample the step runs at (padding included).  The cache holds rows of ONE length, the padded length of the
        forward that filled it; a step at another length would read other samples' rows, so it raises."""
        tc, idx = getattr(self, "_tcache", None), getattr(self, "_mem_index", None)
        if tc is None or idx is None or tc["mem"] is not self.mem_dataloader or len(tc["mem"]) != tc["mem_len"]:
            return None
        layers = list(self.loss_weights.get_distillation_layers())
        if layers != tc["layers"]:
            return None
        if S is not None and int(S) != tc["S"]:
            raise RuntimeError(f"teacher cache: this batch runs at {int(S)} positions per sample, the cache holds rows of {tc['S']} "
                               f"(filled from text length {tc.get('T', '?')}, batch size and text_bucket of build_teacher_cache); "
                               "rebuild the cache for this shape or drop it (drop_teacher_cache)")
        return tc, idx, layers

    def _teacher_rows(self, n_hidden: Optional[int], consumer=None, S: Optional[int] = None):
        """hidden_states[l] of the cached teacher for the batch handed out last as ``ops.TeacherRows`` -- the layer's slab of the cache
        and the batch's sample index within it, which the distillation kernels read in place -- or None when the cache does not cover
        it.  The index is computed here, once per step, on the current stream; ``consumer`` is another stream whose kernels will read
        the rows (the caller's stream when this runs on the teacher's side stream)."""
        got = self._cache_for_batch(S)
        if got is None:
            return None
        tc, idx, layers = got
        states = tc["states"]
        idx = idx.to(states.device)
        index = (idx - tc["lo"]).to(torch.int32)
        if states.is_cuda:
            cur = torch.cuda.current_stream(states.device)
            idx.record_stream(cur)             # (gathered on the loader's stream)
            for st in (cur, consumer):
                # the cache lives on the stream that built it: every other stream that reads it is recorded once, so that a dropped
                # cache (new teacher) is not handed out again while such a reader is still queued
                if st is not None and st not in tc["streams"]:
                    tc["streams"].add(st)
                    states.record_stream(st)
            if consumer is not None:
                index.record_stream(consumer)
        hs = [None] * (max(layers) + 1)
        for k, l in enumerate(layers):
            hs[l] = ops.TeacherRows(states[k], index)
        return hs

    def _cached_teacher_states(self, n_hidden: Optional[int]):
        """hidden_states[l] of the cached teacher for the batch handed out last as dense fp32 tensors (gathered; bf16 rows upcast), or
        None when the cache does not cover it.  The accessor for anything that is not one of the distillation kernels: the step itself
        reads the rows in place (``_teacher_rows``)."""
        got = self._cache_for_batch()
        if got is None:
            return None
        tc, idx, layers = got
        B, S, h = idx.numel(), tc["S"], tc["h"]
        if len(layers) * tc["n"] * S >= 2 ** 31:
            raise RuntimeError(f"teacher cache: {len(layers)} layers x {tc['n']} samples x {S} tokens = {len(layers) * tc['n'] * S} rows exceed "
                               "the 32-bit row ids of the gather kernel")
        rows = (tc["layer_off"] + ((idx.to(tc["ar"].device) - tc["lo"]) * S).view(1, B, 1) + tc["ar"]).to(torch.int32).view(-1)
        out = ops.gather_rows(tc["states"].view(-1, h), rows)          # ONE launch for every distilled layer
        if out.dtype != torch.float32:
            out = ops.cast(out, torch.float32)
        hs = [None] * (max(layers) + 1)
        for k, l in enumerate(layers):
            hs[l] = out[k * B * S: (k + 1) * B * S].view(B, S, h)
        return hs

    def _exact_group(self):
        """The process group of the exact-normaliser all-reduce (``exact_normaliser`` = True: the default group), or None."""
        en = getattr(self, "exact_normaliser", False)
        if not en:
            return None
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
            return None
        return dist.group.WORLD if en is True else en

    def distill(self, output, batch, run=None):
        """``run``: the batch as the engine ran it (replay: _engine_batch) when that is not ``batch`` -- ``output`` and the teacher states
        are then at its text length; the masks left in ``batch`` keep the caller's."""
        layers = self.loss_weights.get_distillation_layers()
        run = batch if run is None else run
        past = self._get_past_hidden_states(batch, n_hidden=max(layers) + 1, run=run)
        dev = output.hidden_states[0].device
        hidden_states = output.hidden_states
        S_in = self.num_vision_tokens + batch["attention_mask"].shape[1]
        fused = (not self._cls_distillation) and self.fused_distill and getattr(output, "mafed_ctx", None) is not None
        if run is not batch and not fused:
            # the per-sample kernels of the generic paths (CLS token, autograd sums) take dense [B, S, h] blocks and the caller's mask:
            # trim the student's states (under autograd: the gradient comes back with zeros behind the text) and the teacher's
            hidden_states = [x[:, :S_in].contiguous() for x in hidden_states]
            if any(isinstance(t, ops.TeacherRows) for t in past):
                past = self._cached_teacher_states(max(layers) + 1)
            past = [t[:, :S_in].contiguous() if t is not None else None for t in past]
            run = batch
        base = self.loss_weights.layer_coeff_vector(dev)
        coeffs = self._cached(("coeffs", id(base), float(self.distillation_coeff)), lambda: (base * float(self.distillation_coeff)).contiguous())
        P = self.num_vision_tokens
        am = batch["attention_mask"].to(dev, torch.int64).contiguous()
        am_run = am if run is batch else run["attention_mask"].to(dev, torch.int64).contiguous()
        if self._cls_distillation:
            if not self._cosine:
                # upstream passes three tensors to MSELoss here and raises
                raise TypeError("cls_distillation requires distillation_loss='cosine'")
            per_layer = torch.stack([_DistillClsFn.apply(hidden_states[l].contiguous(),
                                                         past[l] if isinstance(past[l], ops.TeacherRows) else past[l].contiguous()) for l in layers])
            self.last_modality_losses = None
        else:
            B, T = am.shape
            # side effect kept (distillation.py:139,144): the masks the reference leaves in the batch dict
            zeros_p = self._cached(("zp", B, P, str(dev)), lambda: torch.zeros((B, P), dtype=am.dtype, device=dev))
            batch["lang_masks"] = torch.cat([zeros_p, am], dim=1)
            batch["image_masks"] = self._cached(("im", B, P, T, str(dev)), lambda: torch.cat(
                [torch.ones((B, P), dtype=am.dtype, device=dev), torch.zeros((B, T), dtype=am.dtype, device=dev)], dim=1))
            students = [hidden_states[l] for l in layers]
            teachers = [past[l] for l in layers]
            mctx = getattr(output, "mafed_ctx", None)
            if self.fused_distill and mctx is not None:
                early = getattr(self, "_early", None)
                self._early = None
                if early is not None and (early["layers"] != list(layers) or early["n"] != len(layers)):
                    early = None
                mode, lang_w, lang_vec = self.loss_weights.modality_mode(layers, dev)
                loss, per_layer, modality = _FusedDistillLossFn.apply(
                    mctx[1], am_run, P, teachers, mctx[0], layers, (early["sums"], early["stream"].record_event()) if early is not None else None,
                    coeffs, mode, lang_w, lang_vec, bool(self._cosine), self._exact_group(), *students)
                self.last_modality_losses = modality
                self.last_layer_losses = per_layer
                self.step += 1
                return loss
            sums = _DistillSumsFn.apply(am_run, P, self._cosine, teachers, *students)  # [nl, 4]
            if self._exact_group() is not None:
                counts = global_token_counts(sums.detach(), self._exact_group())[:, 2:4]
                sums = torch.cat([sums[:, 0:2], counts], dim=1)
            lang = sums[:, 0] / sums[:, 2]
            vis = sums[:, 1] / sums[:, 3]
            lw, vw = self.loss_weights.modality_weight_vectors(sums[0, 2].detach(), sums[0, 3].detach(), layers, dev)
            per_layer = lw * lang + vw * vis
            self.last_modality_losses = torch.stack([lang, vis], dim=1).detach()
        self.last_layer_losses = per_layer.detach()
        self.step += 1
        return (coeffs * per_layer).sum()

    # kept for API parity with the reference's per-layer entry point (distillation.py:124-166)
    def feature_distillation(self, batch, hidden_states, past_hidden_states, layer: int):
        dev = hidden_states.device
        if self._cls_distillation:
            return _DistillClsFn.apply(hidden_states.contiguous(), past_hidden_states.contiguous())
        am = batch["attention_mask"].to(dev, torch.int64).contiguous()
        P = self.num_vision_tokens
        sums = _DistillSumsFn.apply(am, P, self._cosine, [past_hidden_states], hidden_states)
        lw, vw = self.loss_weights.modality_weight_vectors(sums[0, 2].detach(), sums[0, 3].detach(), [layer], dev)
        return (lw * sums[:, 0] / sums[:, 2] + vw * sums[:, 1] / sums[:, 3])[0]
