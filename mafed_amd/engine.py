"""The training engine of ``VLPythiaForCausalLM``: the hand-written forward over plain buffers, the hand-scheduled backward sweep and the autograd
node that joins them.  ``EngineMixin`` is a base class of the model (mafed_amd/model.py, which this module does not import): it uses the model's
parameter records, rotary tables and side streams, and the sweep inputs (``contended_backward``, ``grad_overwrite``, ``dw_sumsq`` ...) its
``__init__`` declares.

The forward leaves one record, a dict (``sv`` here, ``st`` at inference callers), which the backward, generation, the distillation plugin, tools
and tests index:
  B, T, T_in, P, S     batch, text length the engine ran at (padded, ``pad_text``) and as given, image positions, S = P + T
  input_ids, attention_mask, labels     as run: at length T
  hidden               [hidden_states[0] .. ] fp32 [B, S, h] views of the residual stream; [L] (post final LayerNorm) only when asked for
  logits, loss         [B, T, V] ([B, 1, V] ``last_only``, [n, V] ``head_rows``, [B, Rc, V] row-sparse) / loss [1]; None when not computed
  layers               per layer, training: {x, mean, rstd, ln1, ln2, qkv, ao, lse, u, a}; ``keep_qkv``: {qkv}; else empty
  training only        proj = (fc, u0, a0) of the projector; final = (xt, lnf, fmean, frstd) of the final LayerNorm; x_last;
                       sparse_head = (slot of every text row, compact labels); head_loss = the backward the forward's head loss returned
                       (``model.head_loss``, mafed_amd/head_loss.py; cross-entropy when the slot is empty): (logits, head labels,
                       dloss [1]) -> dlogits, a closure over what it needs (CE: the lse; logit distillation: teacher logits, lse3, tau,
                       lambda; logit anchor: store, index, lse; squared norm: nothing); the backward sweep pops it
  inject, inject_cosine   written by the fused distillation node before the backward: {layer: (teacher hidden state, device [4] scales)}
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import torch

from mafed_amd import ops
from mafed_amd._lib import EPI_GELU, EPI_GELU_BWD
from mafed_amd.head_loss import CROSS_ENTROPY, HeadLoss


def _trim(x: torch.Tensor, n: int) -> torch.Tensor:
    """The first n positions of a [B, n', ...] tensor as a contiguous tensor (x itself when nothing was appended)."""
    return x if x.shape[1] == n else x[:, :n].contiguous()


@dataclass
class SweepRecord:
    """What a backward sweep reports: left on the model as ``last_sweep`` when the sweep starts, completed as it goes."""
    serial: int = 0                  # counts the model's sweeps: tells a gradient hook which sweep reported a range
    filled_squares: bool = False     # its weight-gradient GEMMs leave the squares of the layers' matrix gradients in ``dw_sumsq``
    dx_chain_event: Optional[torch.cuda.Event] = None   # end of its dX chain; Trainer takes it and resets it to None


class SideWork:
    """Hands parameter-gradient work of a backward sweep to side streams, off the main stream's dX chain.  ``sides`` None: the work runs
    inline.  ``enter(stream)`` is the context that makes ``stream`` current (stubbed by the host test, like the streams themselves)."""

    def __init__(self, main, sides, enter=torch.cuda.stream):
        self.main, self.sides, self.enter = main, sides, enter
        self.keep: List[Any] = []  # temporaries read by the side streams: kept alive until the join
        self._next = 0             # round-robin position over the side streams
        self._mark = None          # event of the main stream's current position; dropped (main_moved) whenever more work is queued on it

    def main_moved(self) -> None:
        self._mark = None

    def on_side(self, fn, *tensors, k: Optional[int] = None) -> None:
        """Run parameter-gradient work after everything queued on the main stream so far, off the dX chain.  Consecutive
        hand-offs with no main-stream work in between share one event: each record is a marker packet the dX chain's next
        kernel waits behind (~4 us apiece in the step's timeline)."""
        sides = self.sides
        if sides is None:
            fn()
            return
        if k is None:
            k = self._next % len(sides)
            self._next += 1
        if self._mark is None:
            self._mark = self.main.record_event()
        with self.enter(sides[k]):
            sides[k].wait_event(self._mark)
            fn()
        self.keep.extend(tensors)

    def after_all(self, fn) -> None:
        """Bucket hook: ``fn`` fires on side stream 0 once every side stream has finished the gradients queued so far."""
        sides = self.sides or ()   # (no side streams: nothing to wait for, and on_side runs `run` inline)
        evs = [st.record_event() for st in sides[1:]]
        def run():
            for e in evs:
                sides[0].wait_event(e)
            fn()
        self.on_side(run, k=0)

    def join(self) -> None:
        if self.sides is not None:
            for st in self.sides:
                self.main.wait_stream(st)  # gradients complete (and `keep` safe to release) from the main stream's point of view
        self.keep.clear()


class BackwardSweep:
    """One backward over an activation record ``sv``: ``head``, ``layer(L-1)`` .. ``layer(0)``, ``projector``, ``finish`` (``run``).  The dX chain
    stays on the caller's stream; parameter gradients go through ``sched`` (SideWork) or, grouped, wait in ``pending_dw`` for ``flush_dw``."""

    def __init__(self, model, sv, dhidden: Sequence[Optional[torch.Tensor]], taps=None):
        self.model, self.sv, self.dhidden, self.taps = model, sv, dhidden, taps
        self.record = model.last_sweep = SweepRecord(model.last_sweep.serial + 1)
        model.final_grad_sumsq = None   # a norm handed over for the buffer as it was (optim.FlatAdamW.clip_grad_norm_) is stale from here on
        cfg = self.cfg = model.config
        self.cd = model.compute_dtype
        self.B, self.T, self.P, self.S = sv["B"], sv["T"], sv["P"], sv["S"]
        self.h, self.L, self.rows = cfg.hidden_size, cfg.num_hidden_layers, self.B * self.S
        self.cos, self.sin = model.rotary_tables(self.S)
        self.wts, self.pars, self.grads = model._tensors(0), model._tensors(1), model._tensors(2)   # compute-dtype weights, fp32 parameters, gradients
        if len(dhidden) > self.L and dhidden[self.L] is not None:
            raise NotImplementedError("gradient w.r.t. the post-final-LayerNorm hidden state is not on the MAFED path")
        self.inject = sv.get("inject")  # {layer: (teacher hidden state, device [4] = d loss / d {sum_lang, sum_vision, ., .})}
        self.inj_cos = bool(sv.get("inject_cosine", False))   # the injected loss is the cosine distance, not the MSE
        self.sched = SideWork(torch.cuda.current_stream(), model.side_streams() if model.overlap_param_grads else None)
        self._decide_policy()
        self.dx = self.dy = None  # gradient w.r.t. the residual stream leaving the current layer, fp32 [rows, h]; the same in compute dtype (GEMM operand)
        self.dy_bias_done = False  # colsum(dy) already accumulated into this layer's two residual-branch bias gradients

    # ---- weight-gradient policy: every decision of the sweep, taken once, before its first launch -------------------------------
    def _decide_policy(self) -> None:
        m, taps = self.model, self.taps
        # layer weight gradients, grouped: (dY, X, gradient) records wait in `pending_dw` (the list keeps dY / X alive) until `flush_dw`
        # (beside collectives the weight gradients go back to one 128 x 128-kernel launch per product on the side streams, as in round 2:
        #  a grouped call would fall back to eight serial launches on the dX chain's stream)
        self.group_dw = (self.cd == torch.bfloat16 and int(m.dw_group_layers) > 0
                         and m.contended_backward in (False, None, "ticketed"))
        # First micro-batch of an accumulation window (Trainer sets ``grad_overwrite``): the grouped weight-gradient GEMMs WRITE the layers'
        # matrix gradients (beta = 0) instead of adding to a zeroed buffer -- the optimiser pass then does not zero-write those 1.2 GB
        # (FlatAdamW: ``skip_matrix_zero``) and the GEMM epilogues do not read them back.  ``_dw_stale`` = the last optimiser pass left the
        # matrices un-zeroed: a sweep that accumulates anyway (another caller, another kernel path) zeroes them first.
        self.overwrite = self.group_dw and bool(m.grad_overwrite) and taps is None
        if m._dw_stale and not self.overwrite:
            m._zero_layer_matrices(range(self.L))
        m._dw_stale = False
        self.dw_beta = 0.0 if self.overwrite else 1.0
        # squares of the final matrix gradients from the weight-gradient epilogues (optim.IncrementalNorm.arm): only a sweep whose
        # products all go through the grouped call can promise them -- its record says so, the norm hook checks it
        self.dw_sq = m.dw_sumsq if (self.group_dw and taps is None) else None
        if self.dw_sq is not None and not m._dw_group_fuses_squares(self.rows):
            self.dw_sq = None   # (h = 768 / 2048: the 256 x 256-tile kernel has no fused squares -- the norm hook's range pass is cheaper than a pass per matrix)
        self.record.filled_squares = self.dw_sq is not None
        self.pending_dw, self.pending_layers = [], []   # product records / layers whose products wait for the next flush
        # deferred LayerNorm parameter reduction: only with side streams and when no external hidden-state gradient adds into the
        # same bias gradients from the main stream (generic autograd path of the cosine / CLS losses)
        self.defer_ln = (self.sched.sides is not None and m.defer_ln_param_reduce and taps is None
                         and not any(d is not None for d in self.dhidden))

    def wgrad(self, dY, X, gw, gb=None) -> None:
        """gw += dY^T . X (and gb += column sums of dY) on a side stream."""
        def run():
            ops.gemm(dY, X, True, False, out=gw, beta=1.0)
            if gb is not None:
                ops.colsum_(dY, gb)
        self.sched.on_side(run, dY, X)

    def wgrad_layer(self, dY, X, i: int, slot: int, with_bias: bool = False) -> None:
        """Weight gradient of layer i's matrix `slot` (0 .. 3 = query_key_value, dense, dense_h_to_4h, dense_4h_to_h: LayerTensors.matrix,
        the order of ``dw_sumsq``), with its bias gradient if asked for."""
        g = self.grads.layers[i]
        gw, gb = g.matrix(slot), g.bias(slot) if with_bias else None
        if not self.group_dw:
            self.wgrad(dY, X, gw, gb)
            return
        q = dict(A=dY, B=X, out=gw, beta=self.dw_beta)
        if self.dw_sq is not None:
            q["sumsq"] = self.dw_sq[i, slot]
        self.pending_dw.append(q)
        if gb is not None:
            self.sched.on_side(lambda: ops.colsum_(dY, gb), dY)

    def flush_dw(self) -> None:
        # at most PP_MAXP = 16 products per grouped launch (mafed_gemm_grouped launches larger lists one product at a time, serially on
        # this stream -- worse than both forms): `dw_group_layers` >= 5 is cut into several launches
        pending = self.pending_dw
        for c0 in range(0, len(pending), 16):
            ops.gemm_grouped(pending[c0:c0 + 16], True, False)
        if pending:
            pending.clear()
            self.sched.main_moved()
        for li in self.pending_layers:
            self.ready(li)
        self.pending_layers.clear()

    def ready(self, i: int) -> None:
        """``grad_ready_hook(i)``, behind every gradient queued so far (SideWork.after_all)."""
        hook = self.model.grad_ready_hook
        if hook is not None:
            self.sched.after_all(lambda: hook(i))

    # ---- stages --------------------------------------------------------------------------------------------------------------
    def run(self, dloss: Optional[torch.Tensor]) -> None:
        self.head(dloss)
        for i in range(self.L - 1, -1, -1):
            self.layer(i)
        self.flush_dw()
        # every layer's LayerNorm / distillation kernel -- the last readers of the teacher's hidden states -- is queued: a consumer
        # that only has to stay behind THOSE (the next step's teacher forward re-uses that memory) can wait for this event instead of
        # for the whole backward, whose side streams still carry ~0.3 ms of parameter-gradient tail
        self.record.dx_chain_event = self.sched.main.record_event()
        self.projector()
        self.finish()

    def head(self, dloss: Optional[torch.Tensor]) -> None:
        """Loss, LM head and final LayerNorm -> ``dx`` / ``dy`` of the last layer's output (None when no loss gradient arrives)."""
        sv, cd, sched = self.sv, self.cd, self.sched
        if dloss is None or sv["loss"] is None:
            return
        B, T, h, V = self.B, self.T, self.h, self.cfg.vocab_size
        Wo, Po, Go = self.wts.outer, self.pars.outer, self.grads.outer
        xt, lnf, fmean, frstd = sv["final"]
        logits = sv["logits"]
        gl = dloss.reshape(1).to(torch.float32).contiguous()
        sp = sv.get("sparse_head")   # (slot of every text row, compact labels): the head ran on the labelled rows only
        n_head = logits.shape[0] * logits.shape[1]
        head_labels = sp[1] if sp is not None else sv["labels"]
        # the backward of this forward's head loss; popped, so that what it holds (a teacher's logits) goes with this call
        dlog = sv.pop("head_loss")(logits, head_labels, gl).view(n_head, V)
        self.wgrad(dlog, lnf, Go.embed_out)
        if cd == torch.bfloat16:
            # [rows, V] . [V, h]: few output tiles with K = 50304 -- accumulate-only fp32 output so that the GEMM splits K
            dlnf = torch.zeros((n_head, h), dtype=torch.float32, device=self.model.flat_params.device)
            ops.gemm(dlog, Wo.embed_out, False, False, out=dlnf, beta=1.0)
        else:
            dlnf = ops.gemm(dlog, Wo.embed_out, False, False)
        if sp is not None:
            dlnf = ops.gather_rows(dlnf if dlnf.dtype == torch.float32 else dlnf.float(), sp[0])   # back to the [B*T, h] text rows (zeros elsewhere)
        if self.defer_ln:
            dxt, _, fws = ops.layernorm_bwd_rows(dlnf, None, xt, fmean, frstd, Po.final_ln_w, None, None)
            sched.main_moved()
            sched.on_side(lambda ws=fws: ops.layernorm_bwd_params(ws, B * T, h, Go.final_ln_w, Go.final_ln_b), fws)
        else:
            dxt, _ = ops.layernorm_bwd(dlnf, None, xt, fmean, frstd, Po.final_ln_w, None, None,
                                       Go.final_ln_w, Go.final_ln_b)
        self.dx, self.dy = ops.pad_text_rows(dxt, B, self.S, self.P, cd if cd != torch.float32 else None)
        sched.main_moved()
        self.ready(self.L)

    def layer(self, i: int) -> None:
        inj = self.inject.get(i) if self.inject else None
        if self._gradient_into(i, inj):
            self._layer_backward(i, inj)

    def _gradient_into(self, i: int, inj) -> bool:
        """``dx`` / ``dy`` of layer i's output with the caller's gradient of hidden_states[i+1] merged in; False: nothing flows into it."""
        sched, dhidden, rows, h, dx = self.sched, self.dhidden, self.rows, self.h, self.dx
        ext = dhidden[i + 1] if (i + 1) < min(len(dhidden), self.L) else None  # grad of hidden_states[i+1] = output of layer i
        if ext is not None:
            ext = ext.reshape(rows, h)
            if dx is not None and self.dy_bias_done:
                # the LayerNorm backward above already added colsum(dx) to this layer's bias gradients: add the rest
                ops.colsum_(ext.to(torch.float32).contiguous(), self.grads.layers[i].fc2_b)
                ops.colsum_(ext.to(torch.float32).contiguous(), self.grads.layers[i].dense_b)
            dx = self.dx = ext.to(torch.float32) if dx is None else dx.add_(ext)
            self.dy = None
            sched.main_moved()
        if dx is None:
            # nothing flows into this layer's output (distillation of shallower layers only): its own backward is skipped,
            # but a distilled hidden_states[i] (this layer's input) still starts the gradient for the layers below
            if inj is not None:
                x = self.sv["layers"][i]["x"].view(self.B, self.S, h)
                self.dx = ops.distill_bwd(x, inj[0], self.sv["attention_mask"], self.P, inj[1], cosine=self.inj_cos).view(rows, h)
                sched.main_moved()
            if self.overwrite:
                self.model._zero_layer_matrices([i])   # (no weight-gradient GEMM will write this layer's matrices in this sweep)
                sched.main_moved()
            return False
        if self.dy is None:
            self.dy = dx if self.cd == torch.float32 else ops.cast(dx, self.cd)
            sched.main_moved()
        return True

    def _layer_backward(self, i: int, inj) -> None:
        sv, cd, sched, cfg, wgrad_layer = self.sv, self.cd, self.sched, self.cfg, self.wgrad_layer
        B, S, P, h, rows, am = self.B, self.S, self.P, self.h, self.rows, sv["attention_mask"]
        dx, dy, dy_bias_done, g = self.dx, self.dy, self.dy_bias_done, self.grads.layers[i]
        H, D, rot = cfg.num_attention_heads, cfg.head_dim, cfg.rotary_ndims
        w, p = self.wts.layers[i], self.pars.layers[i]
        s = sv["layers"][i]
        # parameter gradients that only need dy: MLP down-projection and attention output projection
        wgrad_layer(dy, s["a"], i, 3, with_bias=not dy_bias_done)
        wgrad_layer(dy, s["ao"], i, 1, with_bias=not dy_bias_done)
        # MLP branch
        # (the bias gradients of the two up-projections are column sums of du / dqkv: folded into the producing kernels)
        du = ops.gemm(dy, w.fc2_w, False, False, epilogue=EPI_GELU_BWD, aux=s["u"], colsum=g.fc1_b)
        sched.main_moved()
        wgrad_layer(du, s["ln2"], i, 2)
        dln2 = ops.gemm(du, w.fc1_w, False, False)
        # attention branch
        dao = ops.gemm(dy, w.dense_w, False, False)
        dqkv = ops.attn_bwd(s["qkv"], s["ao"], dao, s["lse"], B, S, H, D, rot, self.cos, self.sin, am, colsum=g.qkv_b)
        sched.main_moved()
        wgrad_layer(dqkv, s["ln1"], i, 0)
        dln1 = ops.gemm(dqkv, w.qkv_w, False, False)
        # both LayerNorms + the residual path, one pass; also emits the compute-dtype copy the next layer's GEMMs read
        ln_kw = dict(want_lp=(cd != torch.float32), teacher=(inj[0].view(rows, h) if torch.is_tensor(inj[0]) else inj[0]) if inj is not None else None,
                     attention_mask=am if inj is not None else None, S=S, P=P, inj_scale=inj[1] if inj is not None else None,
                     inj_mul=-1.0 if self.inj_cos else 2.0 / h)   # (a negative factor selects the cosine-distance gradient, mafed_hip.h)
        below = self.grads.layers[i - 1] if i > 0 else None   # colsum(dx) is the layer below's two residual-branch bias gradients
        dxa, dxb = (below.fc2_b, below.dense_b) if i > 0 else (None, None)
        if self.defer_ln:
            # row kernel on the dX chain; the slab reduction into the LayerNorm / bias gradients goes to a side stream (it feeds
            # parameter gradients only, and on the main stream the whole chip waited for it once per layer)
            dx, dy, ln_ws = ops.layernorm_bwd_rows(dln1, dln2, s["x"], s["mean"], s["rstd"], p.ln1_w, p.ln2_w, dx, want_dxsum=i > 0, **ln_kw)
            sched.main_moved()
            sched.on_side(lambda ws=ln_ws: ops.layernorm_bwd_params(
                ws, rows, h, g.ln1_w, g.ln1_b, g.ln2_w, g.ln2_b, dxa, dxb), ln_ws)
        else:
            dx, dy = ops.layernorm_bwd(dln1, dln2, s["x"], s["mean"], s["rstd"], p.ln1_w, p.ln2_w, dx, g.ln1_w, g.ln1_b, g.ln2_w, g.ln2_b,
                                       dxsum_a=dxa, dxsum_b=dxb, **ln_kw)
            sched.main_moved()
        self.dx, self.dy, self.dy_bias_done = dx, (dx if cd == torch.float32 else dy), i > 0
        if self.taps is not None and i in self.taps:
            self.taps[i] = dx  # = dL/d hidden_states[i] (fresh buffer, never written again on this path)
        if self.group_dw:
            self.pending_layers.append(i)
            if len(self.pending_layers) >= int(self.model.dw_group_layers):
                self.flush_dw()
        else:
            self.ready(i)

    def projector(self) -> None:
        """Token embedding and projector gradients from the gradient of hidden_states[0]."""
        sv, sched, dx = self.sv, self.sched, self.dx
        Wo, Go = self.wts.outer, self.grads.outer
        ext0 = self.dhidden[0] if len(self.dhidden) > 0 else None
        if ext0 is not None:
            ext0 = ext0.reshape(self.rows, self.h)
            dx = ext0.to(torch.float32).contiguous() if dx is None else dx.add_(ext0)
            sched.main_moved()
        if dx is not None:
            fc, u0, a0 = sv["proj"]
            dimg = ops.embed_concat_bwd(dx, sv["input_ids"], self.B, self.P, self.T, self.h, self.cfg.vocab_size, Go.embed_in, self.cd)
            sched.main_moved()
            self.wgrad(dimg, a0, Go.proj2_w, Go.proj2_b)
            du0 = ops.gemm(dimg, Wo.proj2_w, False, False, epilogue=EPI_GELU_BWD, aux=u0, colsum=Go.proj0_b)
            sched.main_moved()
            self.wgrad(du0, fc, Go.proj0_w)

    def finish(self) -> None:
        self.ready(-1)
        self.sched.join()


class EngineMixin:
    """``_engine_forward`` / ``_engine_backward`` and the pieces they are made of, as methods of the model."""

    # ---- forward pieces ----------------------------------------------------------------------------------------------------------
    def _params_ready(self, st, lo: int, hi: int) -> None:
        """Order stream ``st`` behind chunks lo .. hi - 1 of a pipelined optimiser update (``_param_events``, left by
        FlatAdamW.apply_pipelined), numbered -1 = "pre", i = ("layer", i), L = "head"; past the head the events are dropped.  With the
        "pre" chunk the bf16 shadow is refreshed if it is stale."""
        pe, L = self._param_events, self.config.num_hidden_layers
        if pe is not None:
            for c in range(lo, hi):
                st.wait_event(pe["pre" if c < 0 else "head" if c == L else ("layer", c)])
            if hi > L:
                self._param_events = None
        if lo < 0 and self._shadow_dirty:
            self.sync_shadow()

    def _projector_forward(self, feats, n: int, train: bool):
        """Linear -> GELU(erf) -> Linear (vl_pythia.py:226-234,270) over the n * P feature rows -> (fc, u0, a0, img): the features in
        compute dtype, the pre-activation (training only), the activation, the image embeddings."""
        cfg, cd = self.config, self.compute_dtype
        Wo, Po = self._tensors(0).outer, self._tensors(1).outer
        f2 = feats.reshape(n * cfg.num_vision_tokens, cfg.vision_hidden_size)
        if f2.dtype not in (torch.float32, torch.bfloat16):
            f2 = f2.float()
        fc = f2.contiguous() if f2.dtype == cd else ops.cast(f2.contiguous(), cd)
        u0 = torch.empty((f2.shape[0], cfg.hidden_size), dtype=cd, device=fc.device) if train else None
        a0 = ops.gemm(fc, Wo.proj0_w, False, True, bias=Po.proj0_b, epilogue=EPI_GELU, aux=u0)
        return fc, u0, a0, ops.gemm(a0, Wo.proj2_w, False, True, bias=Po.proj2_b)

    def _layer_forward(self, wts, pars, i: int, x: torch.Tensor, attend, qkv_out: Optional[torch.Tensor] = None,
                       rec: Optional[dict] = None, train: bool = False) -> torch.Tensor:
        """Layer i over the fp32 residual rows ``x``: LN pair, fused-QKV product (into ``qkv_out`` when given), ``attend(qkv)`` -> (attention
        output of these rows, its log-sum-exp or None), dense, MLP and the parallel residual -> the next fp32 residual rows.  ``rec`` (a dict)
        receives ``qkv``; under ``train`` also the LayerNorm statistics, the fc1 pre-activation ``u`` and everything else the backward reads."""
        cfg, cd = self.config, self.compute_dtype
        w, p = wts.layers[i], pars.layers[i]
        ln1, ln2, mean, rstd = ops.layernorm_fwd(x, p.ln1_w, p.ln1_b, p.ln2_w, p.ln2_b, cfg.layer_norm_eps, cd, save_stats=train)
        qkv = ops.gemm(ln1, w.qkv_w, False, True, bias=p.qkv_b, out=qkv_out)  # (a captured decode graph reads its K/V cache at fixed addresses)
        ao, lse = attend(qkv)
        # the attention branch output is a bf16 tensor under the reference's autocast too (it meets the fp32 residual in the add)
        attn = ops.gemm(ao, w.dense_w, False, True, bias=p.dense_b, out_dtype=cd)
        u = torch.empty((x.shape[0], cfg.intermediate_size), dtype=cd, device=x.device) if train else None
        a = ops.gemm(ln2, w.fc1_w, False, True, bias=p.fc1_b, epilogue=EPI_GELU, aux=u)
        if rec is not None:
            rec["qkv"] = qkv  # the prefill's K/V cache: exactly what the fused QKV GEMM wrote
            if train:
                rec.update(x=x, mean=mean, rstd=rstd, ln1=ln1, ln2=ln2, ao=ao, lse=lse, u=u, a=a)
        # h + attn(LN1(h)) + mlp(LN2(h)) in the last GEMM's epilogue (tf:271-274)
        return ops.gemm(a, w.fc2_w, False, True, bias=p.fc2_b, out_dtype=torch.float32, res1=attn, res2=x)

    def _final_ln(self, x: torch.Tensor, out_dtype, save_stats: bool = False):
        """Final LayerNorm of fp32 rows -> (rows in ``out_dtype``, None, mean, rstd)."""
        Po = self._tensors(1).outer
        return ops.layernorm_fwd(x, Po.final_ln_w, Po.final_ln_b, None, None, self.config.layer_norm_eps, out_dtype, save_stats=save_stats)

    def _lm_head(self, x: torch.Tensor) -> torch.Tensor:
        """Final LayerNorm + LM head of fp32 rows -> logits [n, V] in compute dtype (inference: no statistics kept)."""
        return ops.gemm(self._final_ln(x, self.compute_dtype)[0], self._tensors(0).outer.embed_out, False, True)

    # ---- engine ------------------------------------------------------------------------------------------------------
    def _engine_forward(self, feats, input_ids, attention_mask, labels, want_hidden, train, n_hidden: Optional[int] = None,
                        keep_qkv: bool = False, qkv_out: Optional[Sequence[torch.Tensor]] = None, label_rows_hint: Optional[int] = None,
                        last_only: bool = False, skip_head: bool = False, pad_text: bool = False, head_rows: Optional[torch.Tensor] = None):
        if not self.flat_params.is_cuda:
            raise RuntimeError("mafed_amd runs on the GPU only (no CPU fallback); move the model with .cuda()")
        pe, main_st = self._param_events, torch.cuda.current_stream()
        self._params_ready(main_st, -1, 0)
        cfg = self.config
        B, T_in = input_ids.shape
        P, h, H, D, L = cfg.num_vision_tokens, cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim, cfg.num_hidden_layers
        # ``pad_text`` (training, evaluation and teacher forwards; not the prefill, whose caches index real positions): masked positions
        # behind the text bring the row count to a tile multiple (text_bucket).  Everything below, the activation record and the
        # backward run at T; the public entry points trim what they hand out to ``T_in``.
        T = self.padded_text_len(B, T_in) if pad_text else T_in
        if T != T_in:
            input_ids, attention_mask, labels = ops.pad_text_batch(input_ids, attention_mask, labels, T)
        S = P + T
        rot = cfg.rotary_ndims
        cos, sin = self.rotary_tables(S)
        wts, pars = self._tensors(0), self._tensors(1)   # compute-dtype weights; fp32 LayerNorm parameters, biases and embedding
        sv: Dict[str, Any] = {"B": B, "T": T, "T_in": T_in, "P": P, "S": S, "input_ids": input_ids, "attention_mask": attention_mask, "labels": labels,
                              "layers": [], "loss": None, "logits": None}
        fc, u0, a0, img = self._projector_forward(feats, B, train)
        x = ops.embed_concat_fwd(img, pars.outer.embed_in, input_ids, B, P, T)  # fp32 residual stream
        if train:
            sv["proj"] = (fc, u0, a0)
        hidden = [x.view(B, S, h)]
        hook = self.hidden_ready_hook if train else None
        if hook is not None:
            hook(0, x)
        attend = lambda qkv: ops.attn_fwd(qkv, B, S, H, D, rot, cos, sin, attention_mask)
        n_layers = L if n_hidden is None else max(0, min(L, n_hidden - 1))
        for i in range(n_layers):
            if pe is not None:
                self._params_ready(main_st, i, i + 1)
            rec = {} if (train or keep_qkv) else None
            if rec is not None:
                sv["layers"].append(rec)
            x = self._layer_forward(wts, pars, i, x, attend, qkv_out[i] if qkv_out is not None else None, rec, train)
            if i < L - 1:
                hidden.append(x.view(B, S, h))
                if hook is not None:
                    hook(i + 1, x)
        sv["hidden"] = hidden
        self._params_ready(main_st, n_layers, L + 1)  # from here on the caller's stream is ordered behind every chunk of the pipelined update
        if n_hidden is not None:
            return sv
        if last_only:
            # a decode prefill only needs the last position's logits: final LN + head on B rows instead of B * T (-> logits [B, 1, V])
            sv["logits"] = self._lm_head(x.view(B, S, h)[:, -1, :].contiguous()).view(B, 1, cfg.vocab_size)
        elif skip_head:
            # representation analysis: hidden_states[L] (the fp32 final-LN state) is the last thing anyone reads; no LM head, no loss
            hidden.append(self._final_ln(x, torch.float32)[0].view(B, S, h))
        elif head_rows is not None:
            # inference (head_logits_rows): final LN + head on the given text rows only -> logits [n, V]; a negative index is a row of zeros
            assert not train and labels is None
            sv["logits"] = self._lm_head(ops.gather_rows(x.view(B, S, h)[:, P:, :].reshape(B * T, h), head_rows))
        else:
            self._head_text(sv, x, feats, want_hidden, train, label_rows_hint)
        return sv

    def _head_text(self, sv, x, feats, want_hidden: bool, train: bool, label_rows_hint: Optional[int]) -> None:
        """final LN (fp32 hidden state L only when asked for) + LM head on the T text positions (vl_pythia.py:89,310) + the loss: the
        row-sparse head where a training batch qualifies, else the dense one."""
        cd = self.compute_dtype
        B, T, P, S, h = sv["B"], sv["T"], sv["P"], sv["S"], self.config.hidden_size
        xt = x.view(B, S, h)[:, P:, :].reshape(B * T, h)
        lnf, _, fmean, frstd = self._final_ln(xt, cd, save_stats=train)
        if want_hidden:
            sv["hidden"].append(self._final_ln(x, torch.float32)[0].view(B, S, h))
        ros, labels, ov = self._head_rows(sv, train, label_rows_hint)
        # the loss: cross-entropy, or on a training forward with labels whatever ``head_loss`` holds (mafed_amd/head_loss.py).  Its
        # ``prepare`` (a teacher's forward) runs on the caller's stream in front of the student's head; its backward goes to
        # BackwardSweep.head through sv["head_loss"]
        hl = None
        if labels is not None:
            hl = self.head_loss if (train and self.head_loss is not None) else CROSS_ENTROPY
            if not isinstance(hl, HeadLoss):
                raise ValueError(f"head_loss must be a mafed_amd.head_loss.HeadLoss or None, got {hl!r}")
            prepared = hl.prepare(feats, sv["input_ids"], sv["attention_mask"], ros)
        if ros is not None:
            lnf = ops.gather_rows(lnf, ros)
        logits = sv["logits"] = ops.gemm(lnf, self._tensors(0).outer.embed_out, False, True).view(B, -1, self.config.vocab_size)
        if train:
            sv["final"] = (xt, lnf, fmean, frstd)
            sv["x_last"] = x
        if hl is not None:
            sv["loss"], parts, backward = hl.forward(logits, labels, ov, prepared)
            if train:
                sv["head_loss"] = backward
            if parts is not None:
                self.last_head_losses = parts

    def _head_rows(self, sv, train: bool, label_rows_hint: Optional[int]):
        """The rows the head runs on -> (row of every slot or None = all T text rows, the head's labels, overflow flag or None).
        Row-sparse head (training, with the caller's bound on labelled positions per sample): only rows whose shifted label is a token
        enter the head GEMM, the loss and -- in the backward -- the head's two gradient GEMMs: 4 answer tokens of 32 text positions in
        the VQA batches, i.e. 256 of 1024 rows at B = 32 (Rc = slots per sample incl. the unlabelled last one, B * Rc a tile multiple)"""
        labels, B, T = sv["labels"], sv["B"], sv["T"]
        Rc = None
        if train and labels is not None and label_rows_hint is not None:
            need = max(2, int(label_rows_hint) + 1)   # (slots per sample incl. the unlabelled last one; a hint of 0 still gets two)
            Rc = need if self.compute_dtype == torch.float32 else next((r for r in range(need, T + 1) if (B * r) % 128 == 0), None)  # (the MFMA tiles want whole 128-row tiles)
            if Rc is not None and Rc * 2 > T:
                Rc = None   # not worth it
        if Rc is None:
            return None, labels, None
        ros, sor, labels, ov = ops.label_rows(labels, Rc)
        # device flag: 1 if a sample had more labelled positions than the hint promised -- rows were dropped; the loss then
        # returns NaN (no host synchronisation: the step fails loudly instead of training on a wrong loss)
        self.last_label_overflow = ov
        sv["sparse_head"] = (sor, labels)
        return ros, labels, ov

    def _dw_group_fuses_squares(self, rows: int) -> bool:
        """Will a grouped weight-gradient launch of this model (``dw_group_layers`` layers x four matrices, K = rows) emit the squares of
        its outputs from the epilogue?  Asked of the library once per (rows, group size)."""
        cache = self._dw_fuse_cache
        key = (int(rows), int(self.dw_group_layers or 0))
        if key not in cache:
            cfg = self.config
            h, f = cfg.hidden_size, cfg.intermediate_size
            per_layer = [(3 * h, h, rows), (h, h, rows), (f, h, rows), (h, f, rows)]
            n_layers = max(1, min(4, key[1]))
            cache[key] = bool(key[1]) and ops.gemm_grouped_fuses_sumsq(per_layer * n_layers, True, False)
        return cache[key]

    def _engine_backward(self, sv, dloss: Optional[torch.Tensor], dhidden: Sequence[Optional[torch.Tensor]], taps=None):
        # Data parallel, last micro-batch of a window: RCCL's all-reduce kernels hold a workgroup per channel for milliseconds while this
        # backward runs.  The persistent GEMMs assume all 256 of their blocks are resident at once -- with 8 CUs taken the late blocks run
        # a second wave and a launch takes 1.7x as long (tools/contention_bench.py: qkv 61.8 -> 105 us, grouped dW 440 -> 785), where the
        # 128 x 128 kernels' many small blocks lose 1.1 - 1.45x.  So this backward runs on those (Trainer sets the flag).
        # (per call: every GEMM this thread issues inside the block carries MAFED_EPI_NO_PERSISTENT; no process-wide switch is touched, a
        #  forced tuning variant or another thread's / model's launches are unaffected)
        cb = self.contended_backward
        if cb and self.flat_params.is_cuda:
            # "ticketed": the persistent kernels stay, their blocks draw tiles from per-XCD queues (MAFED_EPI_TICKETED) -- a launch then
            # tolerates the CUs the collective holds (1.2 - 1.3x instead of 1.7 - 1.9x with 8 - 32 CUs taken, tools/contention_bench.py);
            # True / "128x128": every GEMM of this backward on the 128 x 128 kernels (round 3's choice)
            ctx = ops.ticketed_gemm() if cb == "ticketed" else ops.no_persistent_gemm()
            with ctx:
                return BackwardSweep(self, sv, dhidden, taps).run(dloss)
        return BackwardSweep(self, sv, dhidden, taps).run(dloss)


class _ModelFn(torch.autograd.Function):
    """The whole model as one autograd node: outputs (loss, logits, *hidden_states)."""

    @staticmethod
    def forward(ctx, anchor, model, feats, input_ids, attention_mask, labels, want_hidden, ctx_box, label_rows_hint=None):
        sv = model._engine_forward(feats, input_ids, attention_mask, labels, want_hidden, train=True, label_rows_hint=label_rows_hint, pad_text=True)
        ctx.model, ctx.sv = model, sv
        ctx_box.append(sv)
        ctx.set_materialize_grads(False)  # outputs nobody differentiated arrive as None, not as zero tensors
        # (a 0-dim view of the CE kernel's own output: a clone here was a device copy on the chain between forward and backward)
        loss = sv["loss"].reshape(()) if sv["loss"] is not None else torch.zeros((), device=anchor.device)
        # outs[2] is a 0-dim "hook": the fused distillation node takes it as an input so that this node's backward runs
        # (after the distillation node has left its per-layer coefficients in sv["inject"]) even without a CE gradient; nobody reads
        # its value, so it is not filled
        pub = _trim(sv["logits"], sv["T_in"]) if sv.get("sparse_head") is None else torch.empty(0, device=anchor.device)   # compact logits are internal
        # (one cached zero per device: an uninitialised scalar may hold NaN / Inf, which trips anomaly detection and would propagate if
        #  autograd ever accumulated the hook's gradient with another path; re-using the tensor costs no fill kernel per step)
        outs = [loss, pub.detach(), model._hook_zero().view(())]
        ctx.mark_non_differentiable(outs[1])
        if want_hidden:
            outs += [x.detach() for x in sv["hidden"]]  # aliases: no reference cycle through ctx
        return tuple(outs)

    @staticmethod
    def backward(ctx, dloss, dlogits, dhook, *dhidden):
        sv = ctx.sv
        ctx.sv = None
        if sv is None:
            raise RuntimeError("mafed_amd: backward through the model twice (activations already released)")
        if sv["loss"] is None:
            dloss = None
        ctx.model._engine_backward(sv, dloss, list(dhidden))
        sv.pop("inject", None)
        return (None,) * 9
