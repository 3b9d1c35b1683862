"""GPU: what the shared head-row code (csrc/head_rows.h) makes true by construction.  The cross-entropy forward and ``token_logprob``
call one row log-sum-exp (``row_lse4``) and both end in ``x - (gm + logf(gs))``, so a labelled row's token log-probability is the
row's logit minus the cross-entropy's lse, bit for bit -- one copy of the arithmetic, as tests/test_gpu_mas.py asserts of the penalty
pass that SI and MAS share."""
import pytest
import torch

from tests.test_gpu_kd import _labels

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,T,V", [(2, 3, 512), (3, 5, 1028)])
def test_token_logprob_is_the_logit_minus_the_cross_entropy_lse(B, T, V, dtype):
    from mafed_amd import ops
    g = torch.Generator().manual_seed(B * T + V)
    logits = (torch.randn(B, T, V, generator=g) * 3.0).to(DEV).to(dtype)
    checked = 0
    for first in range(3):   # every rotation of the full / one / none samples
        labels = _labels(B, T, V, first, seed=first).to(DEV)
        target = torch.full((B, T), -100, dtype=torch.int64, device=DEV)
        target[:, :-1] = labels[:, 1:]   # the shifted label; the last position predicts nothing
        _, lse = ops.ce_fwd(logits, labels)
        tlp = ops.token_logprob(logits.view(B * T, V), target.view(-1))
        rows = (target.view(-1) >= 0).nonzero().view(-1)
        x = logits.view(B * T, V)[rows, target.view(-1)[rows]].float()
        want = x - lse.view(-1)[rows]   # torch, fp32
        got = tlp[rows]
        assert got.dtype == torch.float32 and want.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
            f"labels{first}: {int((got.view(torch.int32) != want.view(torch.int32)).sum())} of {rows.numel()} labelled rows differ in bits"
        checked += rows.numel()
    assert checked >= 2 * (T - 1)   # (a full sample in two of the three rotations at least)
