"""Representation-drift analysis: per-layer, per-modality linear CKA between checkpoints (mafed/analysis/).

``feature_space_linear_cka`` is mafed/analysis/cka.py:116-175 on device tensors; ``collect_modality_features`` is the feature
extraction of get_average_CKA_per_layer.py:92-124 (``VLPythiaForCausalLM.modality_features`` per batch); ``modality_cka`` is its
per-run CKA table (:216-225).  The arithmetic runs in the kernels of csrc/cka.hip: fp64 column means and centred row norms once per
feature set, then every centred cross-Gram norm of a call as ONE batched fp32-MFMA launch.  Nothing synchronises with the host.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence

import torch

from mafed_amd import ops


def _debiased(xty, rx, ry, sx, sy, n: int):
    """_debiased_dot_product_similarity_helper (cka.py:103-113), batched over the leading dimensions of the row-norm vectors."""
    return xty - n / (n - 2.0) * (rx * ry).sum(-1) + sx * sy / ((n - 1) * (n - 2))


def _cka(xy, xx, yy, rx=None, ry=None, n: int = 0):
    """CKA from the three HSIC terms (cka.py:136-175); rx / ry: centred squared row norms for the debiased estimator."""
    if rx is None:
        return xy / (xx.sqrt() * yy.sqrt())
    sx, sy = rx.sum(-1), ry.sum(-1)
    return _debiased(xy, rx, ry, sx, sy, n) / (_debiased(xx, rx, rx, sx, sx, n).sqrt() * _debiased(yy, ry, ry, sy, sy, n).sqrt())


def feature_space_linear_cka(features_x: torch.Tensor, features_y: torch.Tensor, debiased: bool = False) -> torch.Tensor:
    """Linear CKA in feature space between fp32 device matrices [n, hx] and [n, hy] (cka.py:116-175); a 0-dim fp64 device tensor."""
    if features_x.dim() != 2 or features_y.dim() != 2 or features_x.shape[0] != features_y.shape[0]:
        raise ValueError(f"expected [n, hx] and [n, hy] feature matrices, got {tuple(features_x.shape)} and {tuple(features_y.shape)}")
    if features_x.dtype != torch.float32 or features_y.dtype != torch.float32:
        raise TypeError("feature_space_linear_cka takes fp32 features (the hidden states are fp32)")
    X, Y = features_x.contiguous(), features_y.contiguous()
    mx, rx = ops.cka_stats(X, row_norms=debiased)
    my, ry = ops.cka_stats(Y, row_norms=debiased)
    h = ops.cka_hsic([(X, mx[0], Y, my[0]), (X, mx[0], X, mx[0]), (Y, my[0], Y, my[0])])
    if debiased:
        return _cka(h[0], h[1], h[2], rx[0], ry[0], X.shape[0])
    return _cka(h[0], h[1], h[2])


def collect_modality_features(model, batches: Iterable[Dict[str, torch.Tensor]], n_samples: Optional[int] = None) -> torch.Tensor:
    """Mean image / mean text hidden state per sample and layer of every batch (get_average_CKA_per_layer.py:92-124) -> fp32
    [2, L, n, h].  A batch holds ``input_ids``, ``attention_mask`` and ``pixel_values`` or ``patch_embeddings``, optionally ``rows``
    (int64 [B], the sample's row in the result: the reference's qid2idx); without ``rows`` the samples fill the rows in order.
    ``n_samples`` defaults to the total batch size."""
    batches = list(batches)
    if n_samples is None:
        n_samples = sum(int(b["input_ids"].shape[0]) for b in batches)
    cfg, dev = model.config, model.flat_params.device
    out = torch.empty((2, cfg.num_hidden_layers, n_samples, cfg.hidden_size), dtype=torch.float32, device=dev)
    row0 = 0
    for b in batches:
        B = int(b["input_ids"].shape[0])
        rows = b.get("rows")
        if rows is None:
            if row0 + B > n_samples:
                raise ValueError(f"{row0 + B} samples do not fit n_samples={n_samples}")
            rows = torch.arange(row0, row0 + B, dtype=torch.int64, device=dev)
        row0 += B
        model.modality_features(b["input_ids"], b["attention_mask"], pixel_values=b.get("pixel_values"),
                                patch_embeddings=b.get("patch_embeddings"), out=out, rows=rows)
    return out


def result_keys(L: int) -> List[str]:
    """The reference's layer keys, image first (get_average_CKA_per_layer.py:100)."""
    return [f"image:{i + 1}" for i in range(L)] + [f"text:{i + 1}" for i in range(L)]


def modality_cka(features: Sequence[torch.Tensor], reference: int = 0, debiased: bool = False) -> Dict[str, torch.Tensor]:
    """CKA of every checkpoint's features against the reference checkpoint's, per modality and layer (get_average_CKA_per_layer.py:
    216-225: feature_space_linear_cka(features[task], features[reference])).  ``features``: one fp32 [2, L, n, h] set per task
    checkpoint.  Returns {"image:1".."image:L", "text:1".."text:L"} -> fp64 [len(features) - 1], tasks in order, the reference
    skipped.  Each set's statistics and self term are computed once; all HSIC terms of the call run as one batch."""
    K = len(features)
    if K < 2 or not 0 <= reference < K:
        raise ValueError(f"need >= 2 checkpoints and 0 <= reference < {K}, got {K} and {reference}")
    two, L, n, h = features[0].shape
    if two != 2 or any(f.shape != features[0].shape or f.dtype != torch.float32 for f in features):
        raise ValueError("every feature set must be fp32 [2, L, n, h] of the same shape")
    feats = [f.contiguous().view(2 * L, n, h) for f in features]
    stats = [ops.cka_stats(f, row_norms=debiased) for f in feats]
    others = [k for k in range(K) if k != reference]
    prods = []
    for k in range(K):   # self terms: K * 2L
        for g in range(2 * L):
            prods.append((feats[k][g], stats[k][0][g], feats[k][g], stats[k][0][g]))
    for k in others:     # cross terms: (K - 1) * 2L, X = the task's features, Y = the reference's (:222)
        for g in range(2 * L):
            prods.append((feats[k][g], stats[k][0][g], feats[reference][g], stats[reference][0][g]))
    hs = ops.cka_hsic(prods)
    self_t = hs[:K * 2 * L].view(K, 2 * L)
    cross = hs[K * 2 * L:].view(K - 1, 2 * L)
    oth = torch.tensor(others, device=hs.device)
    xx, yy = self_t.index_select(0, oth), self_t[reference].expand(K - 1, 2 * L)
    if debiased:
        R = torch.stack([s[1] for s in stats])                          # [K, 2L, n]
        rx, ry = R.index_select(0, oth), R[reference].expand(K - 1, 2 * L, n)
        cka = _cka(cross, xx, yy, rx, ry, n)
    else:
        cka = _cka(cross, xx, yy)
    return {key: cka[:, g].contiguous() for g, key in enumerate(result_keys(L))}
