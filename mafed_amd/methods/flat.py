"""What the plugins that work on the native model's flat buffers share: ``FlatDict``, ``require_native`` and ``behind_optimizer`` (EWC and
the replay family use those too), and ``FlatPlugin``, the base of A-GEM, GEM, SI, MAS, PackNet and TaskMerging."""
from __future__ import annotations

import contextlib
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import torch

from mafed_amd import ops


class FlatDict(dict):
    """name -> view into one flat tensor (``.flat``) laid out like ``model.flat_params``."""

    def __init__(self, model, flat: torch.Tensor):
        super().__init__({name: flat[o:o + n].view(shape) for name, (o, n, shape) in model._offsets.items()})
        self.flat = flat


def require_native(model, who: str, why: str) -> None:
    """Refuse a foreign ``nn.Module``: ``who`` works on the flat buffers, ``why`` says which of them and what for."""
    if not hasattr(model, "flat_params"):
        raise TypeError("%s needs the native model: %s" % (who, why))


def behind_optimizer(model) -> None:
    """Order the caller's stream behind a pipelined optimiser update still in flight: its last chunk's event suffices, all chunks
    share one stream.  The events stay where they are -- the next forward still waits on them layer by layer."""
    pe = getattr(model, "_param_events", None)
    if pe:
        torch.cuda.current_stream().wait_event(list(pe.values())[-1])


class FlatPlugin:
    """Mix-in in front of ``CLStrategy`` / ``ER``: the host-side protocol of a plugin whose passes run on the flat buffers.  A class says
    why it needs them (``_WHY_NATIVE``) and lists its state tensors, each with ``numel(flat_params)`` rows, as ``_STATE`` = ((attribute,
    dtype), ...) in checkpoint order; it sets those attributes to None in its constructor and allocates them when its method says so.
    What depends on the method -- which of them may be None together, what else a checkpoint holds -- stays in the class."""
    grads_only_through_model = False   # a pass of the plugin rewrites the gradient buffer behind the model's backward: handed-over clip norm
    single_process_only = True         # such a pass would have to act on the reduced gradients, which do not exist yet when the hook runs
    #                                    (Trainer refuses a reducer)
    _WHY_NATIVE = "its passes run on the flat buffers (model.flat_params / model.flat_grads)"
    _STATE: Tuple[Tuple[str, torch.dtype], ...] = ()
    _partials: Optional[torch.Tensor] = None   # sum-of-squares partials of the gradient the plugin leaves, for the clip norm
    _segments = _segment_names = _select = None
    _in_view = False

    def _native(self, model) -> torch.Tensor:
        require_native(model, type(self).__name__, self._WHY_NATIVE)
        return model.flat_params

    # ---- the declared state ------------------------------------------------------------------------------------------------
    def _place_state(self, model) -> torch.Tensor:
        """Refuse a state of another model's size and bring what there is of it to the model's device -> ``flat_params``."""
        p = self._native(model)
        for name, _ in self._STATE:
            t = getattr(self, name)
            if t is None:
                continue
            if t.shape[0] != p.numel():
                raise ValueError("%s's state was built for another model (%d elements, this one has %d)" % (type(self).__name__, t.shape[0], p.numel()))
            if t.device != p.device:   # a checkpoint loaded on another device
                setattr(self, name, t.to(p.device))
        return p

    def named(self, model, which: Optional[str] = None) -> FlatDict:
        """name -> view of one state tensor (default: the first the class declares), like EWC's ``fisher[0]``."""
        which = self._STATE[0][0] if which is None else which
        if which not in dict(self._STATE):
            raise KeyError(which)
        self._ensure(model)
        if getattr(self, which) is None:
            raise RuntimeError("%s has no %s allocated" % (type(self).__name__, which))
        return FlatDict(model, getattr(self, which))

    def _state_tensors(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._STATE}

    def _require_keys(self, sd, others: Iterable[str]) -> None:
        missing = [k for k in [name for name, _ in self._STATE] + list(others) if k not in sd]
        if missing:
            raise ValueError("%s state without %s" % (type(self).__name__, missing))

    def _load_tensors(self, sd, names: Sequence[str]) -> None:
        """Every declared tensor named in ``names`` becomes a copy of its own of ``sd``'s (None stays None); the others become None."""
        for name, dtype in self._STATE:
            t = sd[name] if name in names else None
            setattr(self, name, None if t is None else t.detach().to(dtype).clone().contiguous())

    # ---- inside a step -----------------------------------------------------------------------------------------------------
    def compute_loss(self, model, loss, **kwargs):
        return loss

    def _clip_partials(self, like: torch.Tensor, blocks: Callable[[int], int]) -> torch.Tensor:
        """The partials buffer, allocated once per device; ``blocks`` is the ``ops.*_blocks`` of the family whose pass fills it."""
        if self._partials is None or self._partials.device != like.device:
            self._partials = torch.zeros(blocks(like.numel()), dtype=torch.float32, device=like.device)
        return self._partials

    def _hand_over(self, model) -> None:
        model.final_grad_sumsq = self._partials   # FlatAdamW.clip_grad_norm_ folds these instead of reading the buffer again

    # ---- per-tensor selection (PackNet's prune, the TIES trim) --------------------------------------------------------------
    def _segment_tables(self, model, names: List[str], select_blocks: Callable[[int, int], int]):
        """The device table {offset, length} of the tensors ``names`` and the selection's workspaces (blocks per segment, state,
        histogram), built at the first use and again when the names or the device change."""
        dev = model.flat_params.device
        if self._segment_names != names or self._segments.device != dev:
            rows = [[model._offsets[name][0], model._offsets[name][1]] for name in names]
            if any(n >= 2 ** 32 for _, n in rows):
                raise ValueError("%s selects within tensors of fewer than 2^32 elements" % type(self).__name__)
            self._segments = torch.tensor(rows, dtype=torch.int64, device=dev).reshape(len(rows), 2)
            self._segment_names = names
            s = len(rows)
            self._select = (select_blocks(max([n for _, n in rows], default=0), s),
                            torch.zeros(s, 4, dtype=torch.int64, device=dev), torch.zeros(s, ops.PACKNET_BINS, dtype=torch.int32, device=dev))
        return self._segments, self._select

    # ---- parameters replaced for a while -----------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _view(self, model, nests: str, apply: Callable[[], None], prepare: Optional[Callable[[], None]] = None):
        """Inside the block the parameters are what ``apply`` makes of them; on exit they and the shadow are put back bit for bit.
        ``nests`` is the refusal of a view inside a view, ``prepare`` runs behind it and in front of the copy that is put back."""
        if self._in_view:
            raise RuntimeError(nests)
        if prepare is not None:
            prepare()
        behind_optimizer(model)
        p = model.flat_params
        saved = p.detach().clone()
        self._in_view = True
        try:
            apply()
            yield model
        finally:
            self._in_view = False
            with torch.no_grad():
                p.copy_(saved)
            model.sync_shadow()
