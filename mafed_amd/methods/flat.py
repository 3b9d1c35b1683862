"""What the plugins that work on the native model's flat buffers share (EWC, A-GEM, SI, MAS)."""
from __future__ import annotations

import torch


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
