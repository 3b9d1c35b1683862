"""GPU: the fused decode-layer kernels (mafed_amd/csrc/decode.hip) through ``ops.decode_ln_qkv_fc1``, ``ops.decode_ln_linear`` and
``ops.decode_out`` against the fp64 reference of tests/decode_layer_ref.py, element by element within the bound derived there, on
inputs that make a wrong fragment, parameter, row block or K slice visible.  tests/test_decode_layer_ref.py shows on the CPU that this
bound, on these inputs, sees each of those mistakes.  tests/test_gpu_decode.py compares kernel with kernel and stays as it is.

Branch reached by each case (restated from the dispatch in ``decode_layer_ref``: a_form, linear_path, out_plan; asserted per case on the
device's own CU count, the shapes are written for 256 CUs):
  A, direct (variant 760)   h = 256 KS, n1 = 32: (KS, MT) in {1, 2, 3, 4} x {1 .. 4} and (8, 1), (8, 2) at M = 16 MT - 3; M = 16 MT once per
                            KS; the affine parameters load early wherever KS < 8 and MT KS < 16, late else
  A, LDS (761)              h = 1024, M in {5, 16, 29, 32}; M = 33 takes the direct form
  ln_linear                 LDS one-segment form (h = 1024, N = 32 / 96, bias); persistent head at N = 64 CUs and 64 CUs + 32 (unequal trip
                            counts), M in {3, 32}; NP = 4 at h = 256 / 768, N = 256 CUs, M in {7, 20}; NP = 1 at h = 512 and h = 2048 (bias)
  decode_out, direct        h = 256, n1 in {32, 1280, 1408, 1792}: P = 3 (a last slice of one k-step), 12, 13, 16 (second read-back batch),
                            MT 1 .. 4; h = 768 / n1 = 3712 and h = 2048 / n1 = 64: a slice straddles the dense | fc2 seam
  decode_out, LDS           h = 1024, n1 = 512 (P = 3) and 7168 (P = 16), M in {9, 32}; n1 = 7680 (17 slices) falls back to the direct form
Guards on every launch: x (and ao, act) are views whose rows past M hold NaN, the destinations are strided views between sentinels."""
import math

import pytest
import torch

from tests import decode_layer_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7.0


class _variant:
    """mafed_gemm_set_variant(760 / 761): register-direct / LDS-staged operand loads; always back to 761"""
    def __init__(self, lds):
        from mafed_amd import _lib
        self.lib, self.lds = _lib.load(), lds

    def __enter__(self):
        assert self.lib.mafed_gemm_set_variant(761 if self.lds else 760) == 0

    def __exit__(self, *exc):
        self.lib.mafed_gemm_set_variant(761)


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _guarded_rows(t: torch.Tensor) -> torch.Tensor:
    """t [M, K] on the device as the leading rows of a buffer whose three further rows hold NaN"""
    full = torch.full((t.shape[0] + 3, t.shape[1]), math.nan, dtype=t.dtype, device=DEV)
    full[: t.shape[0]] = t.to(DEV)
    return full[: t.shape[0]]


def _ratio(got: torch.Tensor, res) -> float:
    assert got.shape == res["ref"].shape
    assert bool(torch.isfinite(got.float()).all()), "non-finite output"
    return float(((got.double().cpu() - res["ref"]).abs() / res["bound"]).max())


A_PARAMS = [(c, f) for c in R.a_cases() for f in R.A_FAMILIES]


@pytest.mark.parametrize("case,fam", A_PARAMS, ids=[f"{c.id}-{f}" for c, f in A_PARAMS])
def test_ln_qkv_fc1_is_within_the_bound_of_the_fp64_reference(case, fam):
    from mafed_amd import ops
    M, h, n1 = case.M, case.h, case.n1
    assert ops.decode_supported(M, h, n1) and R.a_form(M, h, case.lds)[0] == case.form
    i = R.a_inputs(case, fam)
    qkv, a = R.a_reference(case, fam)
    d = {k: v.to(DEV) for k, v in i.items() if k != "x"}
    x = _guarded_rows(i["x"])
    cache = torch.full((M, 3, 3 * h + 4), SENTINEL, dtype=torch.bfloat16, device=DEV)
    row = cache[:, 1, : 3 * h]
    with _variant(case.lds):
        got_a = ops.decode_ln_qkv_fc1(x, d["g1"], d["b1"], d["g2"], d["b2"], R.EPS, d["wqkv"], d["bqkv"], row, d["w1"], d["bfc1"])
    torch.cuda.synchronize()
    rq, ra = _ratio(row, qkv), _ratio(got_a, a)
    msg = f"[decode-oracle] A {case.form} {fam} M{M} h{h} n1 {n1}: worst err / bound qkv {rq:.3f}, gelu(fc1) {ra:.3f}"
    keep = torch.ones_like(cache, dtype=torch.bool)
    keep[:, 1, : 3 * h] = False
    assert bool((cache[keep] == SENTINEL).all()), "the launch wrote outside the cache row"
    if fam == "census":
        wrong, inside = R.census_check(row.cpu(), qkv["op"], 3 * h)
        msg += f"; census: {wrong} wrong operand elements outside the uncertain set, worst inside it {inside:.2f} ulp"
        print(msg)
        assert wrong == 0 and inside <= 1.0, msg
    else:
        print(msg)
    assert rq <= 1.0 and ra <= 1.0, msg


L_PARAMS = [(c, f) for c in R.l_cases() for f in c.families]


@pytest.mark.parametrize("case,fam", L_PARAMS, ids=[f"{c.id}-{f}" for c, f in L_PARAMS])
def test_ln_linear_is_within_the_bound_of_the_fp64_reference(case, fam):
    from mafed_amd import ops
    M, h, N = case.M, case.h, case.N
    cus = _cus()
    assert R.linear_path(M, h, N, case.bias, cus) == case.path, f"{case.id} does not reach '{case.path}' on {cus} CUs"
    if case.path == "head":
        assert ((N // 16) % cus != 0) == (N != 64 * R.CUS), f"trip counts on {cus} CUs"
    i = R.l_inputs(case, fam)
    res = R.l_reference(case, fam)
    x = _guarded_rows(i["x"])
    buf = torch.full((M, N + 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = buf[:, :N]
    ops.decode_ln_linear(x, i["g"].to(DEV), i["b"].to(DEV), R.EPS, i["w"].to(DEV), bias=None if i["bias"] is None else i["bias"].to(DEV), out=out)
    torch.cuda.synchronize()
    r = _ratio(out, res)
    msg = f"[decode-oracle] ln_linear {case.path} {fam} M{M} h{h} N{N}: worst err / bound {r:.3f}"
    assert bool((buf[:, N:] == SENTINEL).all()), "the launch wrote behind the logits row"
    if fam == "census":
        wrong, inside = R.census_check(out.cpu(), res["op"], N)
        msg += f"; census: {wrong} wrong operand elements outside the uncertain set, worst inside it {inside:.2f} ulp"
        print(msg)
        assert wrong == 0 and inside <= 1.0, msg
    else:
        print(msg)
    assert r <= 1.0, msg


def _run_out(ops, i, M, h, lds):
    """four calls over one workspace, then one in place -> (x', the workspace)"""
    x, ao, act = _guarded_rows(i["x"]), _guarded_rows(i["ao"]), _guarded_rows(i["act"])
    d = {k: i[k].to(DEV) for k in ("wd", "bd", "w2", "b2")}
    ws = ops.decode_out_workspace(M, h, DEV)
    with _variant(lds):
        outs = [ops.decode_out(x, ao, act, d["wd"], d["bd"], d["w2"], d["b2"], ws) for _ in range(4)]
        x2 = x.clone()
        same = ops.decode_out(x2, ao, act, d["wd"], d["bd"], d["w2"], d["b2"], ws, out=x2)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "a repeat gives other bits"
    assert same is x2 and torch.equal(x2, outs[0]), "in place gives other bits"
    assert int(ws[-4 * (h // 32):].view(torch.int32).abs().sum()) == 0, "arrival counters not back at zero"
    return outs[0]


O_PARAMS = [(c, f) for c in R.out_cases() for f in R.OUT_FAMILIES]


@pytest.mark.parametrize("case,fam", O_PARAMS, ids=[f"{c.id}-{f}" for c, f in O_PARAMS])
def test_decode_out_is_within_the_bound_of_the_fp64_reference(case, fam):
    from mafed_amd import ops
    M, h, n1 = case.M, case.h, case.n1
    cus = _cus()
    form, P, ksl = R.out_plan(M, h, n1, cus, case.lds)
    assert ops.decode_supported(M, h, n1) and (form, P) == (case.form, case.P), f"{case.id} lands on {form} P = {P} on {cus} CUs"
    if "straddles" in case.note:
        assert R.straddles(h, P, ksl)
    i, res = R.out_inputs(case, fam), R.out_reference(case, fam)
    got = _run_out(ops, i, M, h, case.lds)
    r = _ratio(got, res)
    print(f"[decode-oracle] decode_out {form} P{P} {fam} M{M} h{h} n1 {n1}: worst err / bound {r:.3f}")
    if fam == "integers":
        assert torch.equal(got.double().cpu(), res["ref"]), "integer operands: every partial sum is exact, so is x'"
    assert r <= 1.0


@pytest.mark.parametrize("h,n1", [(256, 1280), (1024, 512)])
@pytest.mark.parametrize("M", [65, 130])
def test_decode_out_in_blocks_of_64_rows_over_one_workspace(M, h, n1):
    """M > 64: blocks of 64 rows in stream order over the 64-row workspace, the shorter last block on the shifted view whose counters are
    the 64-row layout's.  Integer operands: x' exact."""
    from mafed_amd import ops
    assert ops.decode_supported(M, h, n1)
    i = R.out_operands("integers", M, h, n1)
    res = R.out(**i)
    got = _run_out(ops, i, M, h, True)
    assert torch.equal(got.double().cpu(), res["ref"])
