"""GPU: every inference attention kernel against the fp64 reference of tests/attn_infer_ref.py, element by element within the bound
derived there, on inputs that make one wrong key visible (census, peaked, ascending / descending, masked-max) and at the shapes where
the dispatch changes kernel.  tests/test_attn_infer_ref.py shows on the CPU that this bound, on these inputs, sees a dropped key, a
padded key let in, a neighbour's V row, a rotation one position off, the wrong beam slot and the wrong candidate.

Kernel reached by each case (``Case.path``: attn_decode_launch, attn_decode_beam_go, mfma_ok):
  decode, rotation on load   D = 64 / 80 with rot = 20: scalar; D = 64 / 128 / 256 with rot = D / 4: fused
  decode, pre-rotated cache  fp32, bf16 under variant 740, D = 256: fused; bf16 under 741: flat up to 768 keys (D = 64), 384 keys
                             (D = 128) and Tm = 256, fused at 769 / 385 keys and Tm = 257
  beam                       k = 1, 2: KB 2; k = 3, 4: KB 4; k = 5, 8: KB 8
  suffix, cand               fp32 and bf16 at D = 80: the exact row; bf16 at D = 64 / 128 / 256: MFMA"""
import pytest
import torch

from tests import attn_infer_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(c, f) for c in A.all_cases() for f in A.FAMILIES]


def _dev(x, dtype):
    return x.to(dtype).to(DEV).contiguous()


def _launch(case, inp, ops):
    """One call of the case's kernel on fresh device copies -> (out [rows,H,D] on the CPU, the generated cache after the call or None)"""
    dt = A.DTYPES[case.dtype]
    B, H, D, rot = case.B, case.H, case.D, case.rotary
    cos, sin = (t.to(DEV) for t in A.kernel_tables(inp["cos"], inp["sin"]))
    am = inp["am"].to(DEV)
    new = None
    if case.op in ("decode", "beam"):
        prefix = _dev(inp["prefix"], dt).view(B * case.S0, -1)
        new = _dev(inp["new"], dt).view(inp["new"].shape[0], case.cap, -1)
    if case.op == "decode":
        if case.prerot:
            from mafed_amd import _lib
            lib = _lib.load()
            assert lib.mafed_gemm_set_variant(741 if case.flat else 740) == 0
            try:
                out = ops.attn_decode(prefix, case.S0, new, case.t, B, H, D, rot, cos, sin, am, prerot=True)
            finally:
                lib.mafed_gemm_set_variant(741)
        else:
            out = ops.attn_decode(prefix, case.S0, new, case.t, B, H, D, rot, cos, sin, am)
    elif case.op == "beam":
        out = ops.attn_decode_beam(prefix, case.S0, new, case.t, B, case.k, inp["anc"].to(DEV), H, D, rot, cos, sin, am)
    elif case.op == "suffix":
        N = inp["qkv_img"].shape[0]
        out = ops.attn_suffix_fwd(_dev(inp["qkv_img"], dt).view(N * case.P, -1), inp["index"].to(DEV), N, case.P,
                                  _dev(inp["qkv_txt"], dt).view(B * case.T, -1), case.T, B, H, D, rot, cos, sin, am)
    else:
        out = ops.attn_cand_fwd(_dev(inp["qkv_pre"], dt).view(B * case.S0, -1), case.S0, _dev(inp["qkv_cand"], dt).view(B * case.C * case.A, -1),
                                case.C, case.A, B, H, D, rot, cos, sin, am)
    assert out.dtype == dt
    torch.cuda.synchronize()
    return out.cpu().view(-1, H, D), (None if new is None else new.cpu().view(-1, case.cap, H, 3, D))


def _check_row_t(case, inp, ref, new_after):
    """Pre-rotated cache: the step leaves row t's key rotated, and nothing else of the generated cache moves.  The key is held to one
    ulp of the dtype, eps * (|x c| + |y s|): the kernel evaluates x c -+ y s in fp32 and rounds once more to the dtype, so its error
    scales with the two products, which the result may be far smaller than; the dims that do not rotate are copied."""
    dt = A.DTYPES[case.dtype]
    t, H, D, rot = case.t, case.H, case.D, case.rotary
    before = inp["new"]
    k_got = new_after[:, t, :, 1].double()
    mag = A.rotate_k_operands(before, case.cap, H, D, rot, inp["cos"][case.S0:], inp["sin"][case.S0:])[:, t]
    err = (k_got - ref["k_t"]).abs()
    tol = torch.finfo(dt).eps * mag
    tol[..., rot:] = 0.0
    worst = float((err / tol.clamp(min=1e-300)).max())
    assert bool((err <= tol).all()), f"{case.id}: row t's key after the step is {worst:.3f} ulp off"
    keep = torch.ones_like(before, dtype=torch.bool)
    keep[:, t, :, 1] = False
    assert torch.equal(new_after.double()[keep], before[keep]), "the step wrote more than row t's key (q, v or another row moved)"
    return worst


@pytest.mark.parametrize("case,fam", CASES, ids=[f"{c.id}-{f}" for c, f in CASES])
def test_kernel_is_within_the_bound_of_the_fp64_reference(case, fam):
    from mafed_amd import ops
    dt = A.DTYPES[case.dtype]
    worst, where, worst_key = 0.0, None, 0.0
    for hot in A.variants(case, fam):
        inp = A.build(case, fam, hot)
        ref = A.reference(case, inp)
        bnd = A.bound(ref, case.path, dt)
        got, new_after = _launch(case, inp, ops)
        again, _ = _launch(case, inp, ops)
        assert got.shape == ref["out"].shape
        assert bool(torch.isfinite(got.float()).all()), f"{case.id} {fam} {hot}: non-finite output"
        assert torch.equal(got, again), f"{case.id} {fam} {hot}: a second call gives other bits"
        ratio = (got.double() - ref["out"]).abs() / bnd
        if float(ratio.max()) >= worst:
            worst, where = float(ratio.max()), (hot, [int(i) for i in (ratio == ratio.max()).nonzero()[0]])
        if case.prerot:
            worst_key = max(worst_key, _check_row_t(case, inp, ref, new_after))
    print(f"[attn-infer] {case.path} {fam} {case.shape} {case.dtype}: worst err / bound = {worst:.3f} at {where}"
          + (f"; row t's key: worst err / ulp = {worst_key:.3f}" if case.prerot else ""))
    assert worst <= 1.0, f"{case.id} {fam}: err / bound = {worst:.3f} at (hot key, [row, head, d]) = {where}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_rotate_k_rows_is_the_fp64_rotation(D, dtype):
    """``rotate_k_rows_`` on its own: k within one ulp of the dtype of the fp64 rotation (eps * (|x c| + |y s|), see _check_row_t; the
    dims that do not rotate bit for bit), q and v untouched bit for bit."""
    from mafed_amd import ops
    dt = A.DTYPES[dtype]
    B, S, H, rot = 2, 7, 2, D // 4
    cos, sin = A.tables(D, rot, S)
    x = A.rnd(torch.randn(B, S, H, 3, D, generator=torch.Generator().manual_seed(D), dtype=torch.float64) * 3.0, dtype)
    want = A.rotate_k(x, S, H, D, rot, cos, sin)
    dev = _dev(x, dt).view(B * S, -1)
    kc, ks = (t.to(DEV) for t in A.kernel_tables(cos, sin))
    ops.rotate_k_rows_(dev, B, S, H, D, rot, kc, ks)
    torch.cuda.synchronize()
    got = dev.cpu().view(B, S, H, 3, D).double()
    tol = torch.finfo(dt).eps * A.rotate_k_operands(x, S, H, D, rot, cos, sin)
    tol[..., rot:] = 0.0
    err = (got[:, :, :, 1] - want[:, :, :, 1]).abs()
    print(f"[attn-infer] rotate_k_rows B{B}S{S}H{H}D{D} {dtype}: worst err / ulp = {float((err / tol.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= tol).all())
    assert torch.equal(got[:, :, :, 0], x[:, :, :, 0]) and torch.equal(got[:, :, :, 2], x[:, :, :, 2])
