"""CPU: the float64 yardstick of the LwF head loss (tests/kd_ref.py) against torch's own kl_div / cross_entropy and autograd, and the
registry entry of the plugin."""
import pytest
import torch
import torch.nn.functional as F

from tests.kd_ref import kd_loss, kd_ref, shifted_labels

TOL = 1e-10


def _case(seed, B=3, T=5, V=36, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, T, V, generator=g, dtype=torch.float64) * scale
    t = torch.randn(B, T, V, generator=g, dtype=torch.float64) * scale
    labels = torch.full((B, T), -100, dtype=torch.int64)
    labels[0, 1:] = torch.randint(0, V, (T - 1,), generator=g)   # fully labelled
    labels[1, 3] = V - 1                                         # one labelled row
    return s, t, labels                                          # sample 2: no label at all


def _torch_loss(s, t, labels, tau, lam):
    """The same loss from torch's own building blocks."""
    B, T, V = s.shape
    lab = shifted_labels(labels)
    m = lab != -100
    ce = F.cross_entropy(s.reshape(-1, V), lab.reshape(-1), reduction="none", ignore_index=-100).view(B, T)
    kl = F.kl_div(F.log_softmax(s / tau, -1), F.softmax(t / tau, -1), reduction="none").sum(-1)
    den = m.sum(-1).double().clamp(min=1e-13)
    CE = ((ce * m).sum(-1) / den).mean()
    KD = ((kl * m).sum(-1) / den).mean()
    return CE + lam * tau ** 2 * KD, CE, KD


@pytest.mark.parametrize("tau,lam", [(0.5, 1.0), (1.0, 0.3), (2.0, 1.0), (2.0, 0.0)])
@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_kd_ref_matches_torch_kl_div_and_autograd(tau, lam, scale):
    s, t, labels = _case(3, scale=scale)
    gloss = 1.7
    ref = kd_ref(s, t, labels, tau, lam, gloss=gloss)
    sa = s.clone().requires_grad_(True)
    loss, CE, KD = _torch_loss(sa, t, labels, tau, lam)
    (gloss * loss).backward()
    want = torch.stack([loss, CE, KD]).detach()
    assert float((ref["out3"] - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))
    assert float((ref["dlogits"] - sa.grad).abs().max()) <= TOL
    assert float(ref["dlogits"][2].abs().max()) == 0.0 and float(ref["dlogits"][:, -1].abs().max()) == 0.0
    # the differentiable form used by the model-level oracle is the same arithmetic
    sb = s.clone().requires_grad_(True)
    l2, c2, k2 = kd_loss(sb, t, labels, tau, lam)
    (gloss * l2).backward()
    assert float((torch.stack([l2, c2, k2]).detach() - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))
    assert float((sb.grad - sa.grad).abs().max()) <= TOL
    # saved log-sum-exps: zero on unlabelled rows, torch's on the rest
    m = ref["mask"]
    for i, x in enumerate((s, s / tau, t / tau)):
        assert float(((ref["lse3"][i] - torch.logsumexp(x, -1)) * m).abs().max()) <= TOL * max(1.0, scale / tau)
        assert float((ref["lse3"][i] * ~m).abs().max()) == 0.0


def test_kd_ref_identical_teacher_and_empty_sample():
    s, _, labels = _case(5)
    ref = kd_ref(s, s.clone(), labels, 2.0, 1.0)
    assert float(ref["out3"][2]) == 0.0 and float(ref["out3"][0]) == float(ref["out3"][1])
    none = torch.full_like(labels, -100)
    ref = kd_ref(s, s + 1.0, none, 2.0, 1.0)
    assert float(ref["out3"].abs().max()) == 0.0 and float(ref["dlogits"].abs().max()) == 0.0   # 0, not NaN


def test_lwf_is_registered_with_its_defaults():
    from mafed_amd import CLMethod
    from mafed_amd.methods import CLStrategy
    from mafed_amd.methods.lwf import LwF
    assert "lwf" in CLMethod and CLMethod["lwf"] is LwF and issubclass(LwF, CLStrategy)
    # an extension: constructed through the registry like the reference's entries, listed beside them by names()
    assert CLMethod.get("lwf") is LwF and CLMethod.extensions == {"lwf": LwF} and CLMethod.get("nope") is None
    assert CLMethod.names() == list(CLMethod) + ["lwf"] and "nope" not in CLMethod
    with pytest.raises(KeyError):
        CLMethod["nope"]
    m = CLMethod["lwf"]()
    assert m.reg_lambda == 1.0 and m.temperature == 2.0 and m.task_id == 0 and m.grads_only_through_model
    assert m.replay(None) == (None, 0)
    m = CLMethod["lwf"](reg_lambda=0.3, temperature=0.5)
    assert m.reg_lambda == 0.3 and m.temperature == 0.5
    with pytest.raises(ValueError):
        CLMethod["lwf"](temperature=0.0)
