"""float64 restatement of the LwF head loss (include/mafed_hip.h, mafed_ce_kd_fwd / mafed_ce_kd_bwd).

    CE  = lse(s) - s[lab]                                   per labelled row (shifted label != -100, never the last position)
    KD  = sum_c p_t[c] (t[c] - s[c]) / tau - lse(t / tau) + lse(s / tau),   p_x = softmax(x / tau)
    CE, KD: per sample sum over labelled rows / max(count_b, 1e-13), then the mean over B;  loss = CE + lam tau^2 KD
    dlogits = g_b (softmax(s) - onehot(lab)) + g_b lam tau (p_s - p_t),   g_b = gloss / (B count_b);  zeros on unlabelled rows

``kd_loss`` is the same arithmetic as differentiable torch (for autograd oracles); ``kd_ref`` writes the gradient out by hand.
tests/test_kd_ref.py checks both against torch's own kl_div / cross_entropy and autograd.
"""
import torch


def shifted_labels(labels: torch.Tensor) -> torch.Tensor:
    """lab[b, t] = labels[b, t + 1]; the last position predicts nothing (-100)."""
    lab = torch.full_like(labels, -100)
    lab[:, :-1] = labels[:, 1:]
    return lab


def _rows(s, t, lab, tau):
    V = s.shape[-1]
    lse1 = torch.logsumexp(s, -1)
    lse_s = torch.logsumexp(s / tau, -1)
    lse_t = torch.logsumexp(t / tau, -1)
    ok = (lab >= 0) & (lab < V)
    picked = s.gather(-1, lab.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    ce = torch.where(ok, lse1 - picked, torch.zeros_like(lse1))
    p_t = torch.exp(t / tau - lse_t.unsqueeze(-1))
    kd = (p_t * (t - s) / tau).sum(-1) - lse_t + lse_s
    return ce, kd, (lse1, lse_s, lse_t)


def kd_loss(student: torch.Tensor, teacher: torch.Tensor, labels: torch.Tensor, tau: float, lam: float):
    """(loss, CE, KD) of student / teacher logits [B, T, V] (any float dtype; computed in float64), differentiable in ``student``."""
    s, t = student.double(), teacher.double().detach()
    lab = shifted_labels(labels)
    m = lab != -100
    ce, kd, _ = _rows(s, t, lab, float(tau))
    den = m.sum(-1).double().clamp(min=1e-13)
    zero = torch.zeros_like(ce)
    CE = (torch.where(m, ce, zero).sum(-1) / den).mean()
    KD = (torch.where(m, kd, zero).sum(-1) / den).mean()
    return CE + float(lam) * float(tau) ** 2 * KD, CE, KD


def kd_ref(student: torch.Tensor, teacher: torch.Tensor, labels: torch.Tensor, tau: float, lam: float, gloss: float = 1.0):
    """{"out3" [loss, CE, KD], "lse3" [3, B, T] (0 on unlabelled rows), "dlogits" [B, T, V], "g" [B] = gloss / (B count_b),
    "mask" [B, T]} in float64, from the inputs exactly as given (upcast)."""
    s, t = student.detach().double().cpu(), teacher.detach().double().cpu()
    labels = labels.cpu()
    B, T, V = s.shape
    tau, lam = float(tau), float(lam)
    lab = shifted_labels(labels)
    m = lab != -100
    ce, kd, (lse1, lse_s, lse_t) = _rows(s, t, lab, tau)
    den = m.sum(-1).double().clamp(min=1e-13)
    CE = (ce * m).sum(-1).div(den).mean()
    KD = (kd * m).sum(-1).div(den).mean()
    g = float(gloss) / (B * den)
    onehot = torch.zeros_like(s)
    ok = (lab >= 0) & (lab < V)
    onehot.scatter_(-1, lab.clamp(0, V - 1).unsqueeze(-1), ok.double().unsqueeze(-1))
    p1 = torch.exp(s - lse1.unsqueeze(-1))
    p_s = torch.exp(s / tau - lse_s.unsqueeze(-1))
    p_t = torch.exp(t / tau - lse_t.unsqueeze(-1))
    gb = g.view(B, 1, 1)
    d = (gb * (p1 - onehot) + gb * lam * tau * (p_s - p_t)) * m.unsqueeze(-1)
    lse3 = torch.stack([lse1, lse_s, lse_t]) * m.unsqueeze(0)
    return {"out3": torch.stack([CE + lam * tau ** 2 * KD, CE, KD]), "lse3": lse3, "dlogits": d, "g": g, "mask": m}
