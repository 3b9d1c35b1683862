"""GPU parity of the candidate attention (``ops.attn_cand_fwd``, csrc/attn_cand.hip and attn_cand_mfma_kernel) against rows S0: of
``ops.attn_fwd`` on every assembled [prefix b | candidate (b, c)] sequence.  Inputs as in tests/test_gpu_attn_suffix.py: random qkv,
rot = D / 4, every prompt after the first with some left padding, one prompt with all-padding text."""
import pytest
import torch

from tests.test_gpu_model import DEV, close

pytestmark = pytest.mark.gpu

# (B, P, T, C, A, H, D): one row; several candidates in one tile; 69 rows, candidates straddle a query tile; A > 64; the wider heads;
# the production geometry; two prefix tiles and two query tiles with a candidate straddling them at D = 256
CASES = [
    (2, 8, 6, 1, 1, 2, 64),
    (3, 40, 13, 5, 3, 2, 64),
    (2, 40, 13, 23, 3, 2, 64),
    (2, 8, 6, 2, 70, 1, 64),
    (2, 8, 6, 3, 4, 1, 128),
    (2, 5, 3, 2, 3, 1, 256),
    (4, 256, 32, 8, 6, 16, 64),
    (2, 70, 13, 9, 9, 1, 256),
]


def _case(B, P, T, C, A, H, D, dt):
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + A)
    W = 3 * H * D
    pre = torch.randn(B, P + T, W, generator=g).to(dt).to(DEV)
    cand = torch.randn(B, C, A, W, generator=g).to(dt).to(DEV)
    am = torch.ones(B, T, dtype=torch.int64)
    for b in range(1, B):
        am[b, : 1 + (2 * b) % (T - 1)] = 0   # rows >= 1 carry some left padding
    am[B - 1] = 0                            # one prompt whose text is all padding
    am = am.to(DEV)
    rot = D // 4
    inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    ang = torch.arange(P + T + A, dtype=torch.float32)[:, None] * inv[None, :]
    return pre, cand, am, rot, ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV)


def _full(ops, pre, cand, am, B, P, T, C, A, H, D, rot, cos, sin):
    """Rows S0: of the full forward on the B * C assembled sequences -> [B, C, A, H*D]."""
    S0, S = P + T, P + T + A
    seq = torch.cat([pre[:, None].expand(B, C, S0, -1), cand], dim=2).reshape(B * C * S, -1).contiguous()
    am_x = torch.cat([am.repeat_interleave(C, 0), torch.ones(B * C, A, dtype=torch.int64, device=DEV)], dim=1).contiguous()
    want, _ = ops.attn_fwd(seq, B * C, S, H, D, rot, cos, sin, am_x)
    return want.view(B, C, S, H * D)[:, :, S0:, :]


def _run(ops, pre, cand, am, B, P, T, C, A, H, D, rot, cos, sin):
    return ops.attn_cand_fwd(pre.view(B * (P + T), -1), P + T, cand.view(B * C * A, -1), C, A, B, H, D, rot, cos, sin, am).view(B, C, A, H * D)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,P,T,C,A,H,D", CASES)
def test_attn_cand_equals_the_candidate_rows_of_the_full_attention(dt, B, P, T, C, A, H, D):
    from mafed_amd import ops
    pre, cand, am, rot, cos, sin = _case(B, P, T, C, A, H, D, dt)
    want = _full(ops, pre, cand, am, B, P, T, C, A, H, D, rot, cos, sin)
    got = _run(ops, pre, cand, am, B, P, T, C, A, H, D, rot, cos, sin)
    assert got.dtype == dt and bool(torch.isfinite(got.float()).all())
    close(got.float(), want.float(), 1e-5 if dt == torch.float32 else 2e-2, "candidate attention vs rows S0: of the full forward")
    again = _run(ops, pre, cand, am, B, P, T, C, A, H, D, rot, cos, sin)
    assert torch.equal(got, again), "a second call with the same inputs gives the same bits"


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,P,T,C,A,H,D", [(3, 40, 13, 5, 3, 2, 64), (2, 40, 13, 23, 3, 2, 64), (2, 8, 6, 2, 70, 1, 64), (2, 8, 6, 3, 4, 1, 128)])
def test_attn_cand_rows_do_not_see_other_candidates(dt, B, P, T, C, A, H, D):
    """New tokens in every candidate but c leave out[:, c] bit-identical (c in the middle: neighbours on both sides of it change)."""
    from mafed_amd import ops
    pre, cand, am, rot, cos, sin = _case(B, P, T, C, A, H, D, dt)
    got = _run(ops, pre, cand, am, B, P, T, C, A, H, D, rot, cos, sin)
    c = C // 2
    other = (torch.randn(cand.shape, generator=torch.Generator().manual_seed(7)) * 3.0).to(dt).to(DEV)
    other[:, c] = cand[:, c]
    got2 = _run(ops, pre, other, am, B, P, T, C, A, H, D, rot, cos, sin)
    assert torch.equal(got[:, c], got2[:, c])
    assert not torch.equal(got[:, c - 1], got2[:, c - 1])


def test_attn_cand_rejects_bad_arguments():
    from mafed_amd import _lib
    B, P, T, C, A, H, D = 2, 8, 6, 2, 3, 2, 64
    pre, cand, am, rot, cos, sin = _case(B, P, T, C, A, H, D, torch.float32)
    lib = _lib.load()
    out = torch.empty(B * C * A, H * D, device=DEV)

    def call(S0=P + T, C=C, A=A, T=T, rot=rot, pre=pre, am=am):
        return lib.mafed_attn_cand_fwd(pre.data_ptr() if pre is not None else None, S0, cand.data_ptr(), C, A, _lib.F32, B, H, D, rot, cos.data_ptr(),
                                       sin.data_ptr(), am.data_ptr() if am is not None else None, T, out.data_ptr(), None)

    assert call() == 0
    assert call(T=P + T) != 0 and b"image key" in lib.mafed_last_error_string()      # no image key in front of the text
    assert call(A=0) != 0 and b"bad shape" in lib.mafed_last_error_string()
    assert call(C=0) != 0 and b"bad shape" in lib.mafed_last_error_string()
    assert call(rot=3) != 0 and b"rotary" in lib.mafed_last_error_string()
    assert call(pre=None) != 0 and b"null" in lib.mafed_last_error_string()
    assert call(am=None) != 0 and b"attention_mask" in lib.mafed_last_error_string()
    torch.cuda.synchronize()
