"""Which samples of a finished task go into the replay memory: herding (iCaRL, Rebuffi et al. 2017) and
k-center greedy (Sener & Savarese 2018) in the per-modality feature space MAFED is about -- the per-sample mean image and mean text
hidden state of one layer (``model.pooled_features``).  The greedy loop is ``ops.select_greedy``: one pass over the features per pick,
every pick enqueued from one call, nothing read back in between.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from mafed_amd import ops
from mafed_amd.methods.flat import require_native
from mafed_amd.methods.memory import dataset_len, iter_batches

METHODS = {"herding": ops.SELECT_HERDING, "kcenter": ops.SELECT_KCENTER}
FEATURES = ("both", "image", "text")


def select_rows(X: torch.Tensor, k: int, method: str = "herding", want_scores: bool = False):
    """k rows of X (fp32 [n, d] on the device, read in place) by ``method``, in pick order -> device int64 [k]; a pick is -1 once no
    eligible row is left (a row whose distance is NaN never is).  ``want_scores``: (picks, values fp32 [k], last_scores fp32 [n])
    as ``ops.select_greedy`` returns them.  No synchronisation."""
    if method not in METHODS:
        raise ValueError(f"unknown selection method {method!r} (one of {sorted(METHODS)})")
    mean, _ = ops.cka_stats(X, row_norms=False)
    picks, values, scores = ops.select_greedy(X, mean[0], METHODS[method], k, want_scores=want_scores)
    return (picks, values, scores) if want_scores else picks


class MemorySelection:
    """``selection(model, dataset, k)`` -> the k dataset indices to keep, sorted.

    features: which modality's pooled hidden state spans the space -- ``"both"`` concatenates [image | text] to d = 2 h.
    layer: the decoder layer whose output is pooled (``model.pooled_features``).  normalize: each modality block of a row is scaled
    to unit L2 norm, so that neither modality's scale decides the distance.  batch_size: samples per feature forward (default 32)."""

    def __init__(self, method: str = "herding", features: str = "both", layer: int = -1, normalize: bool = True, batch_size=None):
        if method not in METHODS:
            raise ValueError(f"unknown selection method {method!r} (one of {sorted(METHODS)})")
        if features not in FEATURES:
            raise ValueError(f"unknown feature space {features!r} (one of {FEATURES})")
        self.method, self.feature_space, self.layer, self.normalize = method, features, int(layer), bool(normalize)
        self.batch_size = int(batch_size) if batch_size else 32

    @torch.no_grad()
    def features(self, model, dataset) -> Tuple[torch.Tensor, torch.Tensor]:
        """(X fp32 [n', d], kept int64 [n']) on the model's device: row j of X belongs to sample kept[j].  A sample whose text is empty
        (mask row sum 0: its text mean is NaN by the pooling rule) is dropped.  The masks are summed where the dataset keeps them; with
        a dataset on the host nothing here waits for the GPU."""
        require_native(model, "MemorySelection", "the features come from its inference forward (model.pooled_features)")
        dev, n = model.flat_params.device, dataset_len(dataset)
        pooled = torch.empty((2, n, model.config.hidden_size), dtype=torch.float32, device=dev)
        text_len, lo = [], 0
        for batch in iter_batches(dataset, self.batch_size, ("input_ids", "attention_mask", "patch_embeddings", "pixel_values")):
            b = batch["input_ids"].shape[0]
            images = {key: batch[key] for key in ("patch_embeddings", "pixel_values") if key in batch}
            if "patch_embeddings" in images:
                images.pop("pixel_values", None)
            model.pooled_features(batch["input_ids"], batch["attention_mask"], layer=self.layer, out=pooled,
                                  rows=torch.arange(lo, lo + b, dtype=torch.int64), **images)
            text_len.append(batch["attention_mask"].sum(dim=1).cpu())
            lo += b
        kept = torch.nonzero(torch.cat(text_len) > 0).flatten().to(dev) if n else torch.empty(0, dtype=torch.int64, device=dev)
        blocks = {"both": (0, 1), "image": (0,), "text": (1,)}[self.feature_space]
        parts = []
        for m in blocks:
            x = pooled[m].index_select(0, kept)
            if self.normalize:
                x = x / x.norm(dim=1, keepdim=True)
            parts.append(x)
        X = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        return X.contiguous(), kept

    def __call__(self, model, dataset, k: int) -> np.ndarray:
        X, kept = self.features(model, dataset)
        k = int(k)
        if k > X.shape[0]:
            raise ValueError(f"memory selection: {k} samples asked for, {X.shape[0]} have a text")
        if k == 0:
            return np.empty(0, dtype=np.int64)
        picks = select_rows(X, k, self.method)
        chosen = kept[picks.clamp_min(0)]
        picks_host, chosen_host = torch.stack([picks, chosen]).cpu().numpy()   # the one synchronisation: the dataset is indexed on the host
        if (picks_host < 0).any():
            raise ValueError(f"memory selection: {k} samples asked for, only {int((picks_host >= 0).sum())} have finite features")
        return np.sort(chosen_host)
