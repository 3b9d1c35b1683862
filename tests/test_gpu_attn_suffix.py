"""GPU parity of the shared-image prefill's kernels: ``ops.attn_suffix_fwd`` against rows P .. P+T-1 of ``ops.attn_fwd`` on the
assembled [B, P+T] sequence, and ``ops.prefix_gather`` against torch indexing."""
import pytest
import torch

from tests.test_gpu_model import DEV, close

pytestmark = pytest.mark.gpu

# (B, N, P, T, H, D, image_index): unsorted index with image 1 unused; ragged query tile (T = 33); the production geometry;
# T > 64: a second query tile with its own key-tile count, and waves that skip the tiles behind their rows
CASES = [
    (2, 1, 8, 6, 2, 64, [0, 0]),
    (5, 3, 40, 13, 2, 64, [2, 0, 2, 0, 0]),
    (2, 2, 8, 6, 1, 128, [1, 0]),
    (2, 1, 5, 3, 1, 256, [0, 0]),
    (3, 2, 40, 33, 2, 64, [1, 0, 1]),
    (4, 2, 256, 32, 16, 64, [0, 1, 1, 0]),
    (2, 1, 40, 70, 1, 64, [0, 0]),
    (2, 2, 100, 130, 1, 128, [1, 0]),
]


def _case(B, N, P, T, H, D, index, dt):
    g = torch.Generator().manual_seed(B * 1000 + N * 100 + T)
    W = 3 * H * D
    qkv_img = torch.randn(N, P, W, generator=g).to(dt).to(DEV)
    qkv_txt = torch.randn(B, T, W, generator=g).to(dt).to(DEV)
    am = torch.ones(B, T, dtype=torch.int64)
    for b in range(1, B):
        am[b, : 1 + (2 * b) % (T - 1)] = 0   # every case: rows >= 1 carry some left padding
    if B == 5:
        am[3] = 0                            # one prompt whose text is all padding
    am = am.to(DEV)
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    rot = D // 4
    inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    ang = torch.arange(P + T, dtype=torch.float32)[:, None] * inv[None, :]
    return qkv_img, qkv_txt, am, idx, rot, ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N,P,T,H,D,index", CASES)
def test_attn_suffix_equals_the_text_rows_of_the_full_attention(dt, B, N, P, T, H, D, index):
    from mafed_amd import ops
    qkv_img, qkv_txt, am, idx, rot, cos, sin = _case(B, N, P, T, H, D, index, dt)
    S = P + T
    full = torch.cat([qkv_img[idx], qkv_txt], dim=1).contiguous()   # [B, P+T, 3*H*D]
    want, _ = ops.attn_fwd(full.view(B * S, -1), B, S, H, D, rot, cos, sin, am)
    want = want.view(B, S, H * D)[:, P:, :]
    got = ops.attn_suffix_fwd(qkv_img.view(N * P, -1), idx, N, P, qkv_txt.view(B * T, -1), T, B, H, D, rot, cos, sin, am)
    assert got.shape == (B * T, H * D) and got.dtype == dt
    assert bool(torch.isfinite(got.float()).all())
    close(got.view(B, T, H * D).float(), want.float(), 1e-5 if dt == torch.float32 else 2e-2, "suffix attention vs rows P: of the full forward")
    again = ops.attn_suffix_fwd(qkv_img.view(N * P, -1), idx, N, P, qkv_txt.view(B * T, -1), T, B, H, D, rot, cos, sin, am)
    assert torch.equal(got, again), "a second call with the same inputs gives the same bits"


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,P,T,H,D", [(3, 40, 13, 2, 64), (2, 8, 6, 1, 128)])
def test_attn_suffix_without_an_index_is_the_identity_index(dt, B, P, T, H, D):
    from mafed_amd import ops
    qkv_img, qkv_txt, am, _, rot, cos, sin = _case(B, B, P, T, H, D, list(range(B)), dt)
    ident = torch.arange(B, dtype=torch.int64, device=DEV)
    a = ops.attn_suffix_fwd(qkv_img.view(B * P, -1), None, B, P, qkv_txt.view(B * T, -1), T, B, H, D, rot, cos, sin, am)
    b = ops.attn_suffix_fwd(qkv_img.view(B * P, -1), ident, B, P, qkv_txt.view(B * T, -1), T, B, H, D, rot, cos, sin, am)
    assert torch.equal(a, b)


def test_attn_suffix_rejects_bad_arguments():
    from mafed_amd import _lib, ops
    qkv_img, qkv_txt, am, idx, rot, cos, sin = _case(2, 1, 8, 6, 2, 64, [0, 0], torch.float32)
    with pytest.raises(AssertionError):   # no index: N must equal B
        ops.attn_suffix_fwd(qkv_img.view(8, -1), None, 1, 8, qkv_txt.view(12, -1), 6, 2, 2, 64, rot, cos, sin, am)
    lib = _lib.load()
    rc = lib.mafed_attn_suffix_fwd(qkv_img.data_ptr(), None, 1, 8, qkv_txt.data_ptr(), 6, _lib.F32, 2, 2, 64, rot, cos.data_ptr(), sin.data_ptr(),
                                   am.data_ptr(), qkv_txt.data_ptr(), None)
    assert rc != 0 and b"image_index" in lib.mafed_last_error_string()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_prefix_gather_equals_torch_indexing(dt):
    from mafed_amd import ops
    L, N, B, P, T, W = 3, 2, 5, 8, 6, 384
    g = torch.Generator().manual_seed(9)
    img = torch.randn(L, N * P, W, generator=g).to(dt).to(DEV)
    txt = torch.randn(L, B * T, W, generator=g).to(dt).to(DEV)
    idx = torch.tensor([1, 0, 0, 1, 0], dtype=torch.int64, device=DEV)
    got = ops.prefix_gather(img, txt, idx, B, P, T)
    want = torch.cat([img.view(L, N, P, W)[:, idx], txt.view(L, B, T, W)], dim=2).reshape(L, B * (P + T), W)
    assert got.shape == want.shape and torch.equal(got, want)
    # identity: no index, N == B
    img_b = torch.randn(L, B * P, W, generator=g).to(dt).to(DEV)
    got = ops.prefix_gather(img_b, txt, None, B, P, T)
    want = torch.cat([img_b.view(L, B, P, W), txt.view(L, B, T, W)], dim=2).reshape(L, B * (P + T), W)
    assert torch.equal(got, want)
