"""VLPythia (image-patch prefix + GPT-NeoX decoder) on hand-written gfx950 kernels.

Mirrors the reference model surface for the training hot path:
  * ``model_architecture["vlpythia"]`` registry (mafed/model/__init__.py:3-5)
  * state-dict names/shapes of ``VLCLIPGPTNeoXForCausalLM`` (mafed/model/vl_pythia.py:209-237) so reference
    checkpoints load: ``gpt_neox.embed_in.weight``, ``gpt_neox.layers.{i}.*``, ``gpt_neox.final_layer_norm.*``,
    ``embed_out.weight``, ``vision_embed_tokens.{0,2}.*``
  * ``model(input_ids=, pixel_values=, attention_mask=, labels=, output_hidden_states=, return_dict=True, **kw)``
    -> object with ``.loss``, ``.logits``, ``.hidden_states`` (mafed/model/vl_pythia.py:247-326)

Differences kept deliberately small and documented in DESIGN.md: the frozen vision encoder is the path's input
boundary (``pixel_values`` may be pre-computed ``[B,1+P,Dv]``/``[B,P,Dv]`` features, or a user-supplied frozen
``vision_encoder`` module is called on images); ``.logits`` covers the T text positions only (the reference computes
all S positions and uses the last T, vl_pythia.py:89,310).

The forward/backward of the whole model is ONE autograd node with a hand-scheduled backward (no per-op autograd
graph): activations live in plain buffers, parameter gradients are accumulated by the kernels straight into a flat
fp32 gradient buffer (the RCCL bucket source), hidden-state gradients coming from the distillation loss are injected
at the layer boundaries.
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass, field
from collections import namedtuple
from typing import Any, Dict, List, Optional, Sequence, Tuple

import os as _os

import torch
from torch import nn

from mafed_amd import ops
from mafed_amd.engine import EngineMixin, SweepRecord, _ModelFn, _trim  # noqa: F401  (SweepRecord re-exported)
from mafed_amd.generation import BeamSearchOutput, GenerationMixin, _DecodeCache, _GraphedDecode  # noqa: F401  (re-exported)
from mafed_amd.head_loss import HeadLoss


# ----------------------------------------------------------------------------------------------------------------
@dataclass
class VLPythiaConfig:
    """Fields of config/vlpythia-base.json that the path reads."""

    vocab_size: int = 50304
    hidden_size: int = 1024
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    intermediate_size: int = 4096
    rotary_pct: float = 0.25
    rotary_emb_base: float = 10000.0
    layer_norm_eps: float = 1e-5
    initializer_range: float = 0.02
    vision_hidden_size: int = 1024     # EVA02-L / CLIP-L feature width
    num_vision_tokens: int = 256       # patches kept by feature_select("patch")
    use_parallel_residual: bool = True
    select_feature: str = "patch"

    PRESETS = {"160m": (768, 12, 12), "410m": (1024, 24, 16), "1b": (2048, 16, 8), "1.4b": (2048, 24, 16)}

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @property
    def rotary_ndims(self) -> int:
        return int(self.head_dim * self.rotary_pct)

    @classmethod
    def preset(cls, name: str, **kw) -> "VLPythiaConfig":
        h, L, H = cls.PRESETS[name]
        return cls(hidden_size=h, num_hidden_layers=L, num_attention_heads=H, intermediate_size=4 * h, **kw)

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "VLPythiaConfig":
        keys = {f for f in cls.__dataclass_fields__}
        return cls(**{k: v for k, v in d.items() if k in keys})


@dataclass
class CausalLMOutput:
    """Stand-in for transformers' CausalLMOutputWithPast (mafed/model/vl_pythia.py:320-326)."""

    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past_key_values: Any = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Any = None
    mafed_ctx: Any = None  # (activation record, hook tensor) for the fused distillation path of mafed_amd's own plugin

    def __getitem__(self, i):
        return tuple(v for v in (self.loss, self.logits, self.hidden_states) if v is not None)[i]


# parameter holders: modules without a forward; the tree only exists so that state-dict names match the reference
class _Affine(nn.Module):
    def __init__(self, w: nn.Parameter, b: Optional[nn.Parameter]):
        super().__init__()
        self.weight = w
        if b is not None:
            self.bias = b


class _FrozenVision(nn.Module):
    """Placeholder for the frozen encoder (vqa_cont_learner.py:202-203 freezes ``model.vision_encoder.parameters()``)."""

    def __init__(self, encoder: Optional[nn.Module] = None):
        super().__init__()
        if encoder is not None:
            self.encoder = encoder

    def forward(self, x):
        enc = getattr(self, "encoder", None)
        if enc is None:
            return x
        with torch.no_grad():
            return enc.forward_features(x) if hasattr(enc, "forward_features") else enc(x)


NO_DECAY_KEYS = ("bias", "LayerNorm.bias", "LayerNorm.weight", "vqa_output_distill_loss_params")


def is_no_decay(name: str) -> bool:
    """Name test of BaseModule.configure_optimizers (vqa_cont_learner.py:73-78): GPT-NeoX LayerNorm parameters are
    called ``*layernorm.*`` (lower case), so only names containing ``bias`` escape weight decay."""
    return any(k in name for k in NO_DECAY_KEYS)


# Record field -> state-dict name (behind ``gpt_neox.layers.{i}.`` for a layer's tensors).  In a layer the four (matrix, bias) pairs follow the two
# LayerNorms in slot order 0 .. 3: the order of ``dw_sumsq`` and of ``layer_matrix_range``.
LAYER_FIELD_NAMES = {"ln1_w": "input_layernorm.weight", "ln1_b": "input_layernorm.bias",
                     "ln2_w": "post_attention_layernorm.weight", "ln2_b": "post_attention_layernorm.bias",
                     "qkv_w": "attention.query_key_value.weight", "qkv_b": "attention.query_key_value.bias",
                     "dense_w": "attention.dense.weight", "dense_b": "attention.dense.bias",
                     "fc1_w": "mlp.dense_h_to_4h.weight", "fc1_b": "mlp.dense_h_to_4h.bias",
                     "fc2_w": "mlp.dense_4h_to_h.weight", "fc2_b": "mlp.dense_4h_to_h.bias"}
OUTER_FIELD_NAMES = {"proj0_w": "vision_embed_tokens.0.weight", "proj0_b": "vision_embed_tokens.0.bias",
                     "proj2_w": "vision_embed_tokens.2.weight", "proj2_b": "vision_embed_tokens.2.bias",
                     "embed_in": "gpt_neox.embed_in.weight", "final_ln_w": "gpt_neox.final_layer_norm.weight",
                     "final_ln_b": "gpt_neox.final_layer_norm.bias", "embed_out": "embed_out.weight"}
OuterTensors = namedtuple("OuterTensors", list(OUTER_FIELD_NAMES))   # projector, token embedding, final LayerNorm, LM head


class LayerTensors(namedtuple("LayerTensors", list(LAYER_FIELD_NAMES))):
    """The tensors of one GPT-NeoX layer as views of one flat buffer (weights in compute dtype, fp32 parameters or gradients)."""
    __slots__ = ()

    def matrix(self, slot: int) -> torch.Tensor:
        return self[4 + 2 * slot]

    def bias(self, slot: int) -> torch.Tensor:
        return self[5 + 2 * slot]


def layer_tensor_name(i: int, field: str) -> str:
    return f"gpt_neox.layers.{i}." + LAYER_FIELD_NAMES[field]


def _param_specs(cfg: VLPythiaConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    h, ff, V, dv = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.vision_hidden_size
    layer = LayerTensors((h,), (h,), (h,), (h,), (3 * h, h), (3 * h,), (h, h), (h,), (ff, h), (ff,), (h, ff), (h,))._asdict()
    out: List[Tuple[str, Tuple[int, ...]]] = [("gpt_neox.embed_in.weight", (V, h))]
    out += [(layer_tensor_name(i, f), shape) for i in range(cfg.num_hidden_layers) for f, shape in layer.items()]
    out += [("gpt_neox.final_layer_norm.weight", (h,)), ("gpt_neox.final_layer_norm.bias", (h,)),
            ("embed_out.weight", (V, h)),
            ("vision_embed_tokens.0.weight", (h, dv)), ("vision_embed_tokens.0.bias", (h,)),
            ("vision_embed_tokens.2.weight", (h, h)), ("vision_embed_tokens.2.bias", (h,))]
    return out


class BufferViews:
    """Every tensor of one flat buffer ``src`` as a view: ``layers[i]`` (LayerTensors), ``outer`` (OuterTensors) and ``by_name`` (state-dict
    name -> the same view objects).  Raises if a record field names a tensor that ``offsets`` does not hold, or the records miss one."""
    __slots__ = ("src", "layers", "outer", "by_name")

    def __init__(self, src: torch.Tensor, offsets: Dict[str, Tuple[int, int, Tuple[int, ...]]], n_layers: int):
        self.src = src
        self.by_name = {name: src[o:o + n].view(shape) for name, (o, n, shape) in offsets.items()}
        self.layers = [LayerTensors(*(self.by_name[layer_tensor_name(i, f)] for f in LayerTensors._fields)) for i in range(n_layers)]
        self.outer = OuterTensors(*(self.by_name[name] for name in OUTER_FIELD_NAMES.values()))
        if len(LayerTensors._fields) * n_layers + len(OuterTensors._fields) != len(offsets):
            raise KeyError("the parameter records do not cover every tensor of the flat layout")


TEXT_BUCKET_ROWS = 128      # rows = B * (P + T) that every tiled kernel of the step takes: a multiple of this
TEXT_BUCKET_MAX_PAD = 16    # "auto" appends at most this many positions per sample; a batch that needs more runs unpadded


def bucket_text_len(text_bucket, B: int, P: int, T: int) -> int:
    """Text length T' >= T that a batch of B samples (P image positions each) runs at under the ``text_bucket`` policy:
    ``"auto"``: the smallest T' with B * (P + T') a multiple of TEXT_BUCKET_ROWS if T' - T <= TEXT_BUCKET_MAX_PAD, else T (an odd B, such
    as a short last batch, would need up to 127 positions: left alone); an int m > 0: the smallest T' with (P + T') a multiple of m;
    0: T.  The policy is idempotent: a batch already at T' stays there."""
    if isinstance(text_bucket, str):
        if text_bucket != "auto":
            raise ValueError(f"text_bucket must be 'auto', 0 or a positive int, not {text_bucket!r}")
        for Tp in range(T, T + TEXT_BUCKET_MAX_PAD + 1):
            if (B * (P + Tp)) % TEXT_BUCKET_ROWS == 0:
                return Tp
        return T
    m = int(text_bucket or 0)
    if m < 0:
        raise ValueError(f"text_bucket must be 'auto', 0 or a positive int, not {text_bucket!r}")
    return T if m == 0 else T + (-(P + T)) % m


class VLPythiaForCausalLM(EngineMixin, GenerationMixin, nn.Module):
    """MI355X-native counterpart of ``VLCLIPGPTNeoXForCausalLM`` for the training hot path."""

    def __init__(self, config: VLPythiaConfig, compute_dtype: torch.dtype = torch.bfloat16, device: Any = None,
                 vision_encoder: Optional[nn.Module] = None, seed: Optional[int] = None, text_bucket: Any = None):
        super().__init__()
        assert compute_dtype in (torch.bfloat16, torch.float32)
        # Right padding of the text to a length at which rows = B * (P + T) tile the fast GEMMs (bucket_text_len): "auto" /
        # int / 0 = off.  The engine appends masked positions behind the text and trims what callers see, so only the speed changes.
        # Default: "auto" in bf16; 0 in fp32, whose exact kernels take any shape.
        self.text_bucket = text_bucket if text_bucket is not None else ("auto" if compute_dtype == torch.bfloat16 else 0)
        bucket_text_len(self.text_bucket, 1, 0, 1)   # (a bad value fails here, not in the first step)
        assert config.use_parallel_residual, "GPT-NeoX sequential residual is not on the MAFED path (config/vlpythia-base.json:30)"
        self.config = config
        self.compute_dtype = compute_dtype
        dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        specs = _param_specs(config)
        # flat layout: [decayed ...][non-decayed ...], every tensor starts on a 64-element boundary
        order = [s for s in specs if not is_no_decay(s[0])] + [s for s in specs if is_no_decay(s[0])]
        offs, off = {}, 0
        n_decay_end = 0
        for name, shape in order:
            n = int(math.prod(shape))
            offs[name] = (off, n, shape)
            off += (n + 63) // 64 * 64
            if not is_no_decay(name):
                n_decay_end = off
        self._offsets = offs
        self._n_flat = off
        self._n_decay = n_decay_end
        self.flat_params = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_grads = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_shadow = torch.zeros(off, dtype=torch.bfloat16, device=dev) if compute_dtype == torch.bfloat16 else None
        self._shadow_dirty = True
        self._build_tree(specs)
        from mafed_amd.vision import ClipVisionTower
        if isinstance(vision_encoder, ClipVisionTower):
            # native frozen tower: registered directly so that its tensors appear as ``vision_encoder.vision_model.*``, the names
            # of the reference's state dict (CLIPVisionModel under ``vision_encoder``, vl_pythia.py:215)
            if vision_encoder.config.hidden_size != config.vision_hidden_size or vision_encoder.config.num_patches != config.num_vision_tokens:
                raise ValueError("vision tower (hidden %d, %d patches) does not match the config (vision_hidden_size %d, num_vision_tokens %d)" % (
                    vision_encoder.config.hidden_size, vision_encoder.config.num_patches, config.vision_hidden_size, config.num_vision_tokens))
            self.vision_encoder = vision_encoder
        else:
            self.vision_encoder = _FrozenVision(vision_encoder)
        self._anchor = torch.zeros(1, device=dev, requires_grad=True)
        self._rot_cache: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]] = {}
        # callable(i): fired when layer i's parameter gradients are final for this backward; i = L for the LM head /
        # final LayerNorm, -1 when everything (embeddings, projector) is done.  Used by the DDP bucket reducer.
        self.grad_ready_hook = None
        # callable(l, x): fired in a training forward as soon as hidden_states[l] (fp32 [rows, h]) is final; the MAFED plugin
        # uses it to start that layer's distillation sums on a side stream, under the following layers' GEMMs
        self.hidden_ready_hook = None
        # {"pre" | ("layer", i) | "head": event} left by FlatAdamW.apply_pipelined: the forward waits chunk by chunk
        self._param_events = None
        self._side = None
        self._hook_zero_t: Optional[torch.Tensor] = None   # _hook_zero(): a zero scalar on this replica's device, filled once
        # [weights in compute dtype, fp32 parameters, gradients] as BufferViews: built on first use, dropped by _apply, rebuilt when a flat
        # buffer object was replaced (_tensors)
        self._views: List[Optional[BufferViews]] = [None, None, None]
        self._tensors(1)   # (built here once: a record field that names no tensor of the layout fails at construction, on any machine)
        self.overlap_param_grads = True  # run dW / bias-gradient kernels on side_stream() concurrently with the dX chain
        # bf16: the four weight gradients dW += dY^T.X of `dw_group_layers` consecutive layers are deferred and launched as ONE grouped
        # persistent GEMM (mafed_gemm_grouped) on the main stream: 2 layers = 768 tiles of 128 x 256 = three whole rounds of the
        # 256 CUs without split-K (one layer's products alone leave a third to seven eighths of the chip idle); 0 = one launch each
        self.dw_group_layers = 2
        self._dw_fuse_cache: Dict[Tuple[int, int], bool] = {}   # _dw_group_fuses_squares: (rows, dw_group_layers) -> the library's answer
        self.sparse_lm_head = True          # batches that carry ``max_label_rows`` get the row-sparse LM head in training
        # device flag of the last row-sparse training forward (written there; read by callers / tests): 1 = rows were dropped, the loss is NaN
        self.last_label_overflow: Optional[torch.Tensor] = None
        # The head loss of a training forward with labels (mafed_amd/head_loss.py): None = cross-entropy, else one HeadLoss --
        # LogitDistillation (methods/lwf.py), LogitAnchor (methods/der.py, for one forward), SquaredNorm (methods/mas.py, for its importance
        # pass) or a caller's own.  No other forward looks at it; anything else in it raises in that forward.  Not copied by deepcopy.
        self.head_loss: Optional[HeadLoss] = None
        # device [3] = (loss, CE, KD) of the last training forward under LogitDistillation, or (loss, CE, MSE) under LogitAnchor: the
        # ``parts`` of a head loss that reports some (written there; read by callers, no sync)
        self.last_head_losses: Optional[torch.Tensor] = None
        self.defer_ln_param_reduce = True   # LayerNorm parameter-gradient reduction on a side stream (needs overlap_param_grads)
        # generation (mafed_amd/generation.py)
        self.beam_trace: Optional[List[Any]] = None   # a list: generate(num_beams > 1) appends every step's candidate lists to it
        self.prefill_trace: Optional[List[Any]] = None   # a list: a shared-image prefill (image_index) appends the shapes of its three stores to it
        self.fused_decode = True    # written by callers (tests, tools/decode_bench.py): False = the six-launch decode layer; read when a decode cache is built
        self._decode_graphs: Dict[Tuple, Any] = {}   # written and read by generation._decode (generate / sample with use_graph=True): (B, T, max_new, eos, pad) + the pick object's key -> _GraphedDecode
        # The hand-over of a backward sweep (engine.BackwardSweep).  Its inputs are the attributes below, written by Trainer._device_step and
        # the optimiser before it; what it reports -- its serial, whether its weight-gradient GEMMs fill `dw_sumsq`, the end of its dX chain --
        # is the SweepRecord it leaves in `last_sweep`, which the clip norm (optim.IncrementalNorm) and Trainer read.
        self.contended_backward: Any = False   # Trainer (bench.py, tests) writes: False / None, True / "128x128" or "ticketed" GEMM kernels beside collectives
        self.grad_overwrite = False   # Trainer writes around a window's first backward: the sweep's grouped dW GEMMs write (beta = 0) the matrix gradients
        self._dw_stale = False        # an optimiser pass with skip_matrix_zero sets, the sweep and zero_grad clear: the matrix gradients hold the last window's values
        self.dw_sumsq: Optional[torch.Tensor] = None   # IncrementalNorm.arm / disarm write, the sweep and the norm hook read: fp32 [L, 4, 16] slots of the norm partials
        # sum-of-squares partials of the WHOLE gradient buffer as it now is, left by a pass that wrote it behind the backward (A-GEM's projection):
        # FlatAdamW.clip_grad_norm_ folds them instead of reading the buffer and clears them; every sweep and zero_grad drop them first
        self.final_grad_sumsq: Optional[torch.Tensor] = None
        self.last_sweep = SweepRecord()
        self.reset_parameters(seed)
        self.register_load_state_dict_post_hook(lambda m, ik: setattr(m, "_shadow_dirty", True))

    # ---- construction ---------------------------------------------------------------------------------------
    def _build_tree(self, specs):
        params: Dict[str, nn.Parameter] = {}
        for name, shape in specs:
            o, n, _ = self._offsets[name]
            p = nn.Parameter(self.flat_params[o:o + n].view(shape))
            p.grad = self.flat_grads[o:o + n].view(shape)
            params[name] = p
        self._params_by_name = params
        cfg = self.config
        neox = nn.Module()
        neox.embed_in = _Affine(params["gpt_neox.embed_in.weight"], None)
        layers = nn.ModuleList()
        for i in range(cfg.num_hidden_layers):
            t = LayerTensors(*(params[layer_tensor_name(i, f)] for f in LayerTensors._fields))
            lyr = nn.Module()
            lyr.input_layernorm = _Affine(t.ln1_w, t.ln1_b)
            lyr.post_attention_layernorm = _Affine(t.ln2_w, t.ln2_b)
            att = nn.Module()
            att.query_key_value = _Affine(t.qkv_w, t.qkv_b)
            att.dense = _Affine(t.dense_w, t.dense_b)
            lyr.attention = att
            mlp = nn.Module()
            mlp.dense_h_to_4h = _Affine(t.fc1_w, t.fc1_b)
            mlp.dense_4h_to_h = _Affine(t.fc2_w, t.fc2_b)
            lyr.mlp = mlp
            layers.append(lyr)
        neox.layers = layers
        neox.final_layer_norm = _Affine(params["gpt_neox.final_layer_norm.weight"], params["gpt_neox.final_layer_norm.bias"])
        self.gpt_neox = neox
        self.embed_out = _Affine(params["embed_out.weight"], None)
        vt = nn.Module()
        setattr(vt, "0", _Affine(params["vision_embed_tokens.0.weight"], params["vision_embed_tokens.0.bias"]))
        setattr(vt, "2", _Affine(params["vision_embed_tokens.2.weight"], params["vision_embed_tokens.2.bias"]))
        self.vision_embed_tokens = vt

    def reset_parameters(self, seed: Optional[int] = None):
        """HF init distribution: Linear/Embedding N(0, initializer_range), LayerNorm (1, 0), biases 0."""
        g = torch.Generator(device="cpu")
        g.manual_seed(0 if seed is None else int(seed))
        with torch.no_grad():
            for name, p in self._params_by_name.items():
                if "layernorm" in name or "layer_norm" in name:
                    p.fill_(1.0 if name.endswith("weight") else 0.0)
                elif name.endswith("bias"):
                    p.zero_()
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * self.config.initializer_range)
        self._shadow_dirty = True

    @classmethod
    def from_pretrained(cls, pretrained_model_name: str, vision_encoder_name: str = "", select_layer: int = -2,
                        select_feature: str = "patch", use_flash_attention_2: bool = False, state_dict=None, **kw):
        """Signature of the reference loader (mafed/model/vl_pythia.py:385-394) for a LOCAL directory holding
        ``config.json`` and ``model.safetensors`` / ``pytorch_model.bin``; hub names need network and are refused."""
        import json
        import os
        if not os.path.isdir(pretrained_model_name):
            raise ValueError(f"{pretrained_model_name!r} is not a local directory (no network access on this path)")
        with open(os.path.join(pretrained_model_name, "config.json")) as fp:
            cfg = VLPythiaConfig.from_dict(json.load(fp))
        model = cls(cfg, **kw)
        st = os.path.join(pretrained_model_name, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(pretrained_model_name, "pytorch_model.bin"), map_location="cpu")
        model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("vision_encoder.")}, strict=False)
        if state_dict is not None:
            model.load_state_dict(state_dict, strict=False)
        return model

    def __deepcopy__(self, memo):
        """Teacher snapshot (mafed/methods/distillation.py:211-213): one flat device copy instead of a per-tensor walk."""
        # (the frozen tower is shared, not copied: upstream's deepcopy duplicates ~0.3 B frozen parameters per teacher)
        enc = self.vision_encoder if not isinstance(self.vision_encoder, _FrozenVision) else getattr(self.vision_encoder, "encoder", None)
        new = VLPythiaForCausalLM(self.config, self.compute_dtype, self.flat_params.device, vision_encoder=enc, text_bucket=self.text_bucket)
        with torch.no_grad():
            new.flat_params.copy_(self.flat_params)
        new._shadow_dirty = True
        new.train(self.training)
        return new

    def _apply(self, fn, recurse=True):
        """``.to(device)`` / ``.cuda()``: move the flat buffers and re-point every parameter view at them."""
        probe = fn(self.flat_params)
        if probe.device != self.flat_params.device or probe.dtype != self.flat_params.dtype:
            if probe.dtype != torch.float32:
                raise TypeError("master weights stay fp32; choose compute_dtype at construction")
            self.flat_params = probe
            self.flat_grads = fn(self.flat_grads)
            if self.flat_shadow is not None:
                self.flat_shadow = self.flat_shadow.to(probe.device)
            self._anchor = torch.zeros(1, device=probe.device, requires_grad=True)
            for name, p in self._params_by_name.items():
                o, n, shape = self._offsets[name]
                p.data = self.flat_params[o:o + n].view(shape)
                p.grad = self.flat_grads[o:o + n].view(shape)
            self._rot_cache.clear()
            self._views = [None, None, None]
            self._side = None
            self._shadow_dirty = True
            enc = self.vision_encoder if not isinstance(self.vision_encoder, _FrozenVision) else getattr(self.vision_encoder, "encoder", None)
            if enc is not None:
                enc._apply(fn)
            return self
        return self

    # ---- streams ---------------------------------------------------------------------------------------------------
    N_SIDE = int(_os.environ.get("MAFED_N_SIDE", "3"))   # parameter-gradient streams; same-box A/B on the round-2 build: 1 -> 33.4, 2 -> 34.0, 3 -> 33.4, 4 -> 33.8 ms

    def side_streams(self):
        """Extra HIP streams of this replica: parameter-gradient GEMMs (dW = dY^T.X, bias column sums) run here, off the
        critical dX chain.  Their grids are small (64 / 192 / 256 / 256 tiles per layer at 410M): spread over three
        streams they are co-resident and fill the 512 block slots together with the main stream's kernels."""
        if self._side is None:
            self._side = [torch.cuda.Stream(device=self.flat_params.device) for _ in range(self.N_SIDE)]
        return self._side

    def side_stream(self):
        return self.side_streams()[0]

    def _hook_zero(self) -> torch.Tensor:
        """A zero scalar of this replica's device, filled once (value of the 0-dim hook outputs / gradients nobody reads)."""
        z = self._hook_zero_t
        if z is None or z.device != self.flat_params.device:
            z = self._hook_zero_t = torch.zeros(1, device=self.flat_params.device)
        return z

    # ---- parameter views ---------------------------------------------------------------------------------------
    def sync_shadow(self):
        """Refresh the bf16 copy of the weights read by the MFMA GEMMs (the optimiser kernel keeps it current)."""
        if self.flat_shadow is not None and self.flat_params.is_cuda:
            ops.cast(self.flat_params, torch.bfloat16, out=self.flat_shadow)
        self._shadow_dirty = False

    def _tensors(self, which: int) -> BufferViews:
        """The per-layer / outer records over one flat buffer: 0 = weights in compute dtype (the bf16 shadow, or the parameters in
        fp32 mode), 1 = fp32 parameters, 2 = gradients.  Cached: a call is an index and an identity check, so the engine's pieces fetch them where they need them."""
        src = (self.flat_shadow if self.compute_dtype == torch.bfloat16 else self.flat_params, self.flat_params, self.flat_grads)[which]
        v = self._views[which]
        if v is None or v.src is not src:
            v = self._views[which] = BufferViews(src, self._offsets, self.config.num_hidden_layers)
        return v

    # by state-dict name, for callers outside the engine (tests, tools)
    def _w(self, name: str) -> torch.Tensor:
        """Weight in compute dtype."""
        return self._tensors(0).by_name[name]

    def _p(self, name: str) -> torch.Tensor:
        return self._tensors(1).by_name[name]

    def _g(self, name: str) -> torch.Tensor:
        return self._tensors(2).by_name[name]

    def zero_grad(self, set_to_none: bool = False):  # gradients are views of the flat buffer: always zero in place
        self.flat_grads.zero_()
        self._dw_stale = False
        self.final_grad_sumsq = None

    def layer_matrix_range(self, i: int) -> Tuple[int, int]:
        """Flat range of layer i's four weight matrices (query_key_value, dense, dense_h_to_4h, dense_4h_to_h: contiguous, behind the layer's
        two LayerNorm weights in the decayed segment) -- the part of the gradient buffer that the grouped weight-gradient GEMMs write whole."""
        grads = self._tensors(2)
        first = [grads.layers[i].matrix(slot).storage_offset() - grads.src.storage_offset() for slot in range(4)]
        lo, o, n = first[0], first[3], grads.layers[i].matrix(3).numel()
        assert all(lo <= k < o + n for k in first)
        return lo, o + (n + 63) // 64 * 64

    def _zero_layer_matrices(self, layers) -> None:
        for i in layers:
            lo, hi = self.layer_matrix_range(i)
            self.flat_grads[lo:hi].zero_()

    def decay_split(self) -> int:
        """flat[:n] is weight-decayed, flat[n:] is not."""
        return self._n_decay

    def rotary_tables(self, S: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """cos/sin [S, rot/2] fp32 (GPTNeoXRotaryEmbedding, tf:52-108; positions = arange(S), pads not skipped)."""
        key = (S, str(self.flat_params.device))
        if key not in self._rot_cache:
            rd = self.config.rotary_ndims
            inv = 1.0 / (self.config.rotary_emb_base ** (torch.arange(0, rd, 2, dtype=torch.float32) / rd))
            fr = torch.arange(S, dtype=torch.float32)[:, None] * inv[None, :]
            self._rot_cache[key] = (fr.cos().contiguous().to(self.flat_params.device), fr.sin().contiguous().to(self.flat_params.device))
        return self._rot_cache[key]

    # ---- public forward ------------------------------------------------------------------------------------------
    def get_patch_embeddings(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """get_patch_embeddings + feature_select (mafed/model/vl_pythia.py:453-475): images [B,3,H,W] go through the frozen
        tower (the native CLIP tower of mafed_amd.vision, or a user-supplied module); features pass through."""
        P, dv = self.config.num_vision_tokens, self.config.vision_hidden_size
        x = pixel_values
        if x.dim() == 4:
            x = self.vision_encoder(x)
        if x.dim() != 3 or x.shape[-1] != dv:
            raise ValueError(f"expected vision features [B,{P}(+1),{dv}], got {tuple(x.shape)}")
        if x.shape[1] == P + 1 and self.config.select_feature == "patch":
            x = x[:, 1:]
        if x.shape[1] != P:
            raise ValueError(f"expected {P} patch tokens, got {x.shape[1]}")
        return x

    def forward(self, input_ids: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None,
                attention_mask: Optional[torch.Tensor] = None, position_ids=None, inputs_embeds=None, head_mask=None,
                past_key_values=None, labels: Optional[torch.Tensor] = None, use_cache=None, output_attentions=None,
                output_hidden_states: Optional[bool] = None, return_dict: Optional[bool] = None,
                allow_input_gradients: bool = False, patch_embeddings: Optional[torch.Tensor] = None, **kwargs):
        if input_ids is None or (pixel_values is None and patch_embeddings is None):
            raise ValueError("the training path needs input_ids and pixel_values / patch_embeddings")
        if position_ids is not None or inputs_embeds is not None or past_key_values is not None or use_cache or output_attentions:
            raise NotImplementedError("position_ids / inputs_embeds / KV cache / attentions are outside the MAFED training path")
        feats = patch_embeddings if patch_embeddings is not None else self.get_patch_embeddings(pixel_values)
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        want_h = bool(output_hidden_states)
        dev = self.flat_params.device
        input_ids = input_ids.to(dev, torch.int64).contiguous()
        attention_mask = attention_mask.to(dev, torch.int64).contiguous()
        labels = labels.to(dev, torch.int64).contiguous() if labels is not None else None
        feats = feats.to(dev).contiguous()
        if torch.is_grad_enabled():
            ctx_box: List[Any] = []
            # ``max_label_rows`` (an int the replay buffer attaches to its batches): upper bound on the labelled positions of a sample ->
            # row-sparse LM head (loss and gradients unchanged; ``.logits`` is None then: nothing on the training path reads it)
            hint = kwargs.get("max_label_rows") if (self.sparse_lm_head and labels is not None) else None
            outs = _ModelFn.apply(self._anchor, self, feats, input_ids, attention_mask, labels, want_h, ctx_box, hint)
            loss = outs[0] if labels is not None else None
            # (the node's hidden states are the engine's own, at the padded length: trimmed here, under autograd, so that a gradient a
            #  caller sends into one comes back with zeros at the appended positions)
            S_in = ctx_box[0]["P"] + ctx_box[0]["T_in"]
            logits, hs = (outs[1] if outs[1].numel() else None), tuple(_trim(x, S_in) for x in outs[3:]) if want_h else None
            mctx = (ctx_box[0], outs[2]) if want_h else None
        else:
            mctx = None
            st = self._engine_forward(feats, input_ids, attention_mask, labels, want_h, train=False, pad_text=True)
            loss = st["loss"].reshape(()) if st["loss"] is not None else None
            logits, hs = _trim(st["logits"], st["T_in"]), tuple(_trim(x, st["P"] + st["T_in"]) for x in st["hidden"]) if want_h else None
        out = CausalLMOutput(loss=loss, logits=logits, hidden_states=hs, mafed_ctx=mctx)
        if return_dict is False:
            return tuple(v for v in (out.loss, out.logits, out.hidden_states) if v is not None)
        return out

    def padded_text_len(self, B: int, T: int) -> int:
        """The text length a [B, T] batch runs at under this model's ``text_bucket`` (bucket_text_len)."""
        return bucket_text_len(self.text_bucket, int(B), self.config.num_vision_tokens, int(T))

    def padded_candidate_len(self, n: int, A: int) -> int:
        """The length n candidates of A tokens run at in ``score`` under ``text_bucket``: the policy of ``padded_text_len`` on rows without an
        image part (``"auto"``: n * A' a multiple of TEXT_BUCKET_ROWS when that takes at most TEXT_BUCKET_MAX_PAD positions)."""
        return bucket_text_len(self.text_bucket, int(n), 0, int(A))

    def pad_text_batch(self, input_ids, attention_mask, labels=None):
        """(ids, mask, labels) of a [B, T] batch on this model's device at ``padded_text_len(B, T)``: one launch, or the tensors themselves
        when nothing is appended.  What every engine entry does with its batch; a caller that feeds the same batch to two models (student
        and frozen teacher) pads once and passes the result to both -- a batch at the padded length is left alone."""
        dev = self.flat_params.device
        input_ids = input_ids.to(dev, torch.int64).contiguous()
        attention_mask = attention_mask.to(dev, torch.int64).contiguous()
        labels = labels.to(dev, torch.int64).contiguous() if labels is not None else None
        B, T = input_ids.shape
        Tp = self.padded_text_len(B, T)
        if Tp == T:
            return input_ids, attention_mask, labels
        return ops.pad_text_batch(input_ids, attention_mask, labels, Tp)

    @torch.no_grad()
    def hidden_states_upto(self, input_ids, attention_mask, pixel_values=None, patch_embeddings=None, n_hidden: Optional[int] = None):
        """Frozen-teacher fast path (mafed/methods/distillation.py:218-224): hidden_states[0 .. n_hidden-1] only --
        the stack stops after layer n_hidden-2, no LM head, no saved activations."""
        feats = patch_embeddings if patch_embeddings is not None else self.get_patch_embeddings(pixel_values)
        dev = self.flat_params.device
        st = self._engine_forward(feats.to(dev).contiguous(), input_ids.to(dev, torch.int64).contiguous(),
                                  attention_mask.to(dev, torch.int64).contiguous(), None, True, train=False, n_hidden=n_hidden, pad_text=True)
        return tuple(_trim(x, st["P"] + st["T_in"]) for x in st["hidden"])

    @torch.no_grad()
    def modality_features(self, input_ids, attention_mask, pixel_values=None, patch_embeddings=None, out: Optional[torch.Tensor] = None,
                          rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-sample mean image and mean text hidden state of every layer 1..L (mafed/analysis/get_average_CKA_per_layer.py:107-118):
        one inference forward without the LM head, then one pooling launch.  out fp32 [2 (image, text), L, n, h] (allocated with
        n = B if None); sample b lands in row rows[b] (default b).  The text mean is over the LAST sum(attention_mask[b]) positions,
        the reference's literal rule (the same rows as the mask's under left padding); an empty text gives NaN."""
        feats = patch_embeddings if patch_embeddings is not None else self.get_patch_embeddings(pixel_values)
        cfg, dev = self.config, self.flat_params.device
        input_ids = input_ids.to(dev, torch.int64).contiguous()
        attention_mask = attention_mask.to(dev, torch.int64).contiguous()
        B = input_ids.shape[0]
        if out is None:
            out = torch.empty((2, cfg.num_hidden_layers, B, cfg.hidden_size), dtype=torch.float32, device=dev)
        if rows is not None:
            rows = rows.to(dev, torch.int64).contiguous()
        st = self._engine_forward(feats.to(dev).contiguous(), input_ids, attention_mask, None, True, train=False, skip_head=True)
        ops.cka_pool(st["hidden"][1:], attention_mask, cfg.num_vision_tokens, out, rows)
        return out

    @torch.no_grad()
    def pooled_features(self, input_ids, attention_mask, pixel_values=None, patch_embeddings=None, layer: int = -1,
                        out: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``modality_features(...)[:, layer]`` without the other layers: the inference forward stops behind decoder layer ``layer``
        (0 .. L-1, negative from the end; the last one ends in the final LayerNorm, as hidden_states[L] does), no LM head, then one
        pooling launch over that one hidden state.  out fp32 [2 (image, text), n, h] (allocated with n = B if None); sample b lands
        in row rows[b] (default b).  The same launches as ``modality_features`` up to that layer, hence the same bits."""
        feats = patch_embeddings if patch_embeddings is not None else self.get_patch_embeddings(pixel_values)
        cfg, dev = self.config, self.flat_params.device
        L = cfg.num_hidden_layers
        if not -L <= int(layer) < L:
            raise IndexError(f"layer {layer} outside [-{L}, {L})")
        layer = int(layer) % L
        input_ids = input_ids.to(dev, torch.int64).contiguous()
        attention_mask = attention_mask.to(dev, torch.int64).contiguous()
        B = input_ids.shape[0]
        if out is None:
            out = torch.empty((2, B, cfg.hidden_size), dtype=torch.float32, device=dev)
        assert out.dim() == 3 and out.is_contiguous()
        if rows is not None:
            rows = rows.to(dev, torch.int64).contiguous()
        last = layer == L - 1
        st = self._engine_forward(feats.to(dev).contiguous(), input_ids, attention_mask, None, True, train=False,
                                  n_hidden=None if last else layer + 2, skip_head=last)
        ops.cka_pool(st["hidden"][-1:], attention_mask, cfg.num_vision_tokens, out.unsqueeze(1), rows)
        return out

    @torch.no_grad()
    def head_logits_rows(self, feats, input_ids, attention_mask, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Inference logits of a batch that is already at its padded length (pad_text_batch), for a frozen teacher: the stack, the final
        LayerNorm and the LM head on the text rows ``rows`` only (int32 indices into the [B * T] text rows; a negative one gives a row
        of zeros) -> [len(rows), V] in compute dtype; ``rows`` None -> [B, T, V].  No activations are kept."""
        dev = self.flat_params.device
        if rows is not None:
            rows = rows.to(dev, torch.int32).contiguous()
        st = self._engine_forward(feats.to(dev).contiguous(), input_ids.to(dev, torch.int64).contiguous(),
                                  attention_mask.to(dev, torch.int64).contiguous(), None, False, train=False, head_rows=rows)
        return st["logits"]

    @torch.no_grad()
    def answer_logits(self, feats, input_ids, attention_mask, labels, A: int) -> torch.Tensor:
        """Inference logits on the labelled rows of a batch, in rank order, for a store of answer logits (methods/der.py) -> [B, A, V] in
        compute dtype: slot j of sample b holds the logits of b's j-th labelled row (the row whose shifted label is its j-th token), unused
        slots hold zeros.  The engine's own text padding, the stack, then the final LayerNorm and the LM head on those rows only; no
        activations are kept.  A sample with more than ``A`` labelled rows raises (one host read of a device flag: between tasks)."""
        A = int(A)
        if A < 1:
            raise ValueError(f"answer_logits: A must be at least 1, got {A}")
        input_ids, attention_mask, labels = self.pad_text_batch(input_ids, attention_mask, labels)
        B = input_ids.shape[0]
        ros, _, _, ov = ops.label_rows(labels, A + 1)   # (slots per sample incl. the unlabelled last one)
        rows = ros.view(B, A + 1)[:, :A].reshape(-1)
        n = B * A
        if self.compute_dtype == torch.bfloat16 and n % 128:   # (whole MFMA tiles: the rest are rows of zeros, dropped below)
            rows = torch.nn.functional.pad(rows, (0, 128 - n % 128), value=-1)
        out = self.head_logits_rows(feats, input_ids, attention_mask, rows)[:n].view(B, A, self.config.vocab_size)
        # (a negative row is a zero hidden state, whose logits are the final LayerNorm's bias through the head: not zeros yet)
        out.masked_fill_((rows[:n] < 0).view(B, A, 1), 0)
        if int(ov.item()):
            raise ValueError(f"answer_logits: a sample has more than A = {A} labelled rows")
        return out

    def hidden_grad_taps(self, batch: Dict[str, torch.Tensor], layers: Sequence[int]) -> Dict[int, torch.Tensor]:
        """dL_CE / d hidden_states[l] for every l in ``layers`` from ONE backward sweep (the adaptive-weights pass of
        mafed/methods/distillation_loss_weights.py:91-146 asks autograd for them one layer at a time)."""
        feats = batch["patch_embeddings"] if "patch_embeddings" in batch else self.get_patch_embeddings(batch["pixel_values"])
        dev = self.flat_params.device
        sv = self._engine_forward(feats.to(dev).contiguous(), batch["input_ids"].to(dev, torch.int64).contiguous(),
                                  batch["attention_mask"].to(dev, torch.int64).contiguous(),
                                  batch["labels"].to(dev, torch.int64).contiguous(), False, train=True, pad_text=True)
        taps: Dict[int, torch.Tensor] = {int(l): None for l in layers}
        self._engine_backward(sv, torch.ones(1, device=dev), [], taps=taps)
        S = sv["S"]
        return {l: _trim(t.view(sv["B"], S, -1), sv["P"] + sv["T_in"]) for l, t in taps.items()}


model_architecture = {"vlpythia": VLPythiaForCausalLM}
