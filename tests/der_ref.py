"""float64 restatement of the DER++ head loss (include/mafed_hip.h, mafed_ce_mse_fwd / mafed_ce_mse_bwd).

    CE  = lse(s) - s[lab]                          per labelled row (shifted label != -100, never the last position)
    MSE = (1 / V) sum_c (s[c] - z[c])^2,           z = store[mem_index[b], j(b, t)],  j = the rank of row t among b's labelled rows
    CE, MSE: per sample sum over labelled rows / max(count_b, 1e-13), then the mean over B;  loss = beta CE + alpha MSE
    dlogits = g_b (beta (softmax(s) - onehot(lab)) + alpha (2 / V) (s - z)),   g_b = gloss / (B count_b);  zeros on unlabelled rows

``der_loss`` is the same arithmetic as differentiable torch (for autograd oracles); ``der_ref`` writes the gradient out by hand.
tests/test_der_ref.py checks one against the other.  The rank map is a plain Python loop.
"""
import torch

from tests.kd_ref import shifted_labels


def rank_map(labels: torch.Tensor):
    """[(b, t, j)]: labelled row t of sample b is the j-th labelled row of that sample (j = 0 for the first)."""
    lab = shifted_labels(labels.cpu())
    out = []
    for b in range(lab.shape[0]):
        j = 0
        for t in range(lab.shape[1]):
            if int(lab[b, t]) != -100:
                out.append((b, t, j))
                j += 1
    return out


def gather_targets(store: torch.Tensor, mem_index: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """z [B, T, V] float64: the stored row of every labelled head row, zeros elsewhere.  An index outside the store raises."""
    B, T = labels.shape
    n_mem, A, V = store.shape
    z = torch.zeros(B, T, V, dtype=torch.float64)
    st = store.detach().double().cpu()
    for b, t, j in rank_map(labels):
        m = int(mem_index[b])
        if not (0 <= m < n_mem and j < A):
            raise IndexError(f"row ({b}, {t}): store[{m}, {j}] outside [{n_mem}, {A}]")
        z[b, t] = st[m, j]
    return z


def _rows(s, z, lab):
    V = s.shape[-1]
    lse = torch.logsumexp(s, -1)
    ok = (lab >= 0) & (lab < V)
    picked = s.gather(-1, lab.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    ce = torch.where(ok, lse - picked, torch.zeros_like(lse))
    mse = ((s - z) ** 2).sum(-1) / V
    return ce, mse, lse


def der_loss(student: torch.Tensor, store: torch.Tensor, mem_index: torch.Tensor, labels: torch.Tensor, alpha: float, beta: float):
    """(loss, CE, MSE) of student logits [B, T, V] against ``store`` [n_mem, A, V] (any float dtype; computed in float64),
    differentiable in ``student``."""
    s = student.double()
    labels = labels.cpu()
    z = gather_targets(store, mem_index, labels).to(s.device)
    lab = shifted_labels(labels).to(s.device)
    m = lab != -100
    ce, mse, _ = _rows(s, z, lab)
    den = m.sum(-1).double().clamp(min=1e-13)
    zero = torch.zeros_like(ce)
    CE = (torch.where(m, ce, zero).sum(-1) / den).mean()
    MSE = (torch.where(m, mse, zero).sum(-1) / den).mean()
    return float(beta) * CE + float(alpha) * MSE, CE, MSE


def der_ref(student: torch.Tensor, store: torch.Tensor, mem_index: torch.Tensor, labels: torch.Tensor, alpha: float, beta: float,
            gloss: float = 1.0):
    """{"out3" [loss, CE, MSE], "lse" [B, T] (0 on unlabelled rows), "dlogits" [B, T, V], "g" [B] = gloss / (B count_b), "mask" [B, T],
    "dmax" = max |s - z| over the labelled rows} in float64, from the inputs exactly as given (upcast)."""
    s = student.detach().double().cpu()
    labels = labels.cpu()
    B, T, V = s.shape
    alpha, beta = float(alpha), float(beta)
    z = gather_targets(store, mem_index, labels)
    lab = shifted_labels(labels)
    m = lab != -100
    ce, mse, lse = _rows(s, z, lab)
    den = m.sum(-1).double().clamp(min=1e-13)
    CE = (ce * m).sum(-1).div(den).mean()
    MSE = (mse * m).sum(-1).div(den).mean()
    g = float(gloss) / (B * den)
    onehot = torch.zeros_like(s)
    ok = (lab >= 0) & (lab < V)
    onehot.scatter_(-1, lab.clamp(0, V - 1).unsqueeze(-1), ok.double().unsqueeze(-1))
    p = torch.exp(s - lse.unsqueeze(-1))
    diff = (s - z) * m.unsqueeze(-1)
    d = g.view(B, 1, 1) * (beta * (p - onehot) + alpha * (2.0 / V) * diff) * m.unsqueeze(-1)
    return {"out3": torch.stack([beta * CE + alpha * MSE, CE, MSE]), "lse": lse * m, "dlogits": d, "g": g, "mask": m,
            "dmax": float(diff.abs().max()) if diff.numel() else 0.0}
