"""CPU: the fp64 reference of the fused decode-layer kernels (tests/decode_layer_ref.py) pinned to torch's fp64 layer_norm / gelu, the
uncertain-element model checked against fp32 LayerNorms in three summation orders, the 1 % cap on every case of the GPU list, and the
guard that the bound of tests/test_gpu_decode_oracle.py can see the mistakes it is there for: every mutation below, applied to the
reference on the very inputs the GPU tests run, moves at least one element by more than twice the bound (the kernel's own permitted
error cannot hide it), or breaks the bit-exact census / integers property."""
import pytest
import torch
import torch.nn.functional as F

from tests import decode_layer_ref as R

F64 = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# pin
# ------------------------------------------------------------------------------------------------------------------------------
def test_reference_is_torch_fp64_layer_norm_and_gelu():
    g = torch.Generator().manual_seed(0)
    M, h, n1 = 5, 256, 64
    x = torch.randn(M, h, generator=g, dtype=F64) * 1.7 + 0.4
    g1, b1, g2, b2 = (torch.randn(h, generator=g, dtype=F64) for _ in range(4))
    _close(R.layer_norm(x, g1, b1, 1e-5), F.layer_norm(x, (h,), g1, b1, 1e-5))
    u = torch.linspace(-9, 9, 1001, dtype=F64)
    _close(R.gelu(u), F.gelu(u))
    wqkv, w1 = R.grid_weight(3 * h, h, g), R.grid_weight(n1, h, g, gain=0.5)
    bqkv, bfc1 = R.col_bias(3 * h, g), R.col_bias(n1, g)
    qkv, a = R.ln_qkv_fc1(x, g1, b1, g2, b2, 1e-5, wqkv, bqkv, w1, bfc1)
    y1, y2 = F.layer_norm(x, (h,), g1, b1, 1e-5), F.layer_norm(x, (h,), g2, b2, 1e-5)
    _close(qkv["ref"], R.bf16_round(y1) @ wqkv.double().t() + bqkv.double())
    _close(a["ref"], F.gelu(R.bf16_round(y2) @ w1.double().t() + bfc1.double()))
    lin = R.ln_linear(x, g1, b1, 1e-5, wqkv, None)
    _close(lin["ref"], R.bf16_round(y1) @ wqkv.double().t())
    i = R.out_operands("random", M, h, n1)
    want = i["x"].double() + F.linear(i["ao"].double(), i["wd"].double(), i["bd"].double()) + F.linear(i["act"].double(), i["w2"].double(), i["b2"].double())
    _close(R.out(**i)["ref"], want)


def test_bf16_round_is_round_to_nearest_even_on_eight_bits():
    v = torch.tensor([1.0, 1.00390625, 1.01171875, -1.00390625, 255.5, 256.5 + 0.5, 0.0, 3.0e-3], dtype=F64)
    want = torch.tensor([1.0, 1.0, 1.015625, -1.0, 256.0, 256.0, 0.0, float(torch.tensor(3.0e-3).to(torch.bfloat16))], dtype=F64)
    assert torch.equal(R.bf16_round(v), want)
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 3      # fp32 values: torch's own fp32 -> bf16 is one rounding
    assert torch.equal(R.bf16_round(x.double()), x.to(torch.bfloat16).double())
    assert float(R.half_ulp(torch.tensor([1.5], dtype=F64), 8)) == 2.0 ** -8 and float(R.half_ulp(torch.tensor([1.5], dtype=F64), 24)) == 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------------------
# the uncertain set holds every flip of an fp32 LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------
def _ln32_direct_order(x, g, b, eps):
    """decode_ln_qkv_fc1_kernel's order in fp32: k = wave (32 KS) + 32 u + 8 g + e; a tree inside a fragment, the lane's KS fragments in
    turn, the four g lanes by xor 1 and 2, the eight waves in turn; the centred squares the same way"""
    M, h = x.shape
    ks = h // 256

    def fold(v):                                   # v [M, 8, KS, 4, 8] fp32
        f = ((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])) + ((v[..., 4] + v[..., 5]) + (v[..., 6] + v[..., 7]))
        s = f[:, :, 0]
        for u in range(1, ks):
            s = s + f[:, :, u]
        s = (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])
        t = s[:, 0]
        for w in range(1, 8):
            t = t + s[:, w]
        return t[:, None]

    v = x.view(M, 8, ks, 4, 8)
    mean = fold(v) / h
    d = x - mean
    rstd = 1.0 / torch.sqrt(fold((d * d).view(M, 8, ks, 4, 8)) / h + eps)
    return ((x - mean) * rstd) * g + b


def _ln32_lds_order(x, g, b, eps):
    """the LDS forms' order: lane l takes columns 4 (l + 64 jj) .. + 3, a pair tree per jj, jj in turn, six xor shuffles"""
    M, h = x.shape

    def fold(v):                                   # v [M, KS, 64, 4]
        s = 0
        for jj in range(v.shape[1]):
            s = s + ((v[:, jj, :, 0] + v[:, jj, :, 1]) + (v[:, jj, :, 2] + v[:, jj, :, 3]))
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, torch.arange(64) ^ o]
        return s[:, :1]

    mean = fold(x.view(M, -1, 64, 4)) / h
    d = x - mean
    rstd = 1.0 / torch.sqrt(fold((d * d).view(M, -1, 64, 4)) / h + eps)
    return ((x - mean) * rstd) * g + b


@pytest.mark.parametrize("fam", ["distinct", "edge"])
@pytest.mark.parametrize("h", [256, 1024, 2048])
def test_fp32_layernorm_flips_only_uncertain_elements(h, fam):
    g = torch.Generator().manual_seed(h)
    x = R.rows(fam, 64, h, g)
    gm, bt = R.ln_params(h, g)
    op = R.normalised(x, gm, bt, R.EPS)
    flips = 0
    for name, y32 in (("torch", F.layer_norm(x, (h,), gm, bt, R.EPS)), ("direct", _ln32_direct_order(x, gm, bt, R.EPS)), ("lds", _ln32_lds_order(x, gm, bt, R.EPS))):
        assert y32.dtype == torch.float32
        assert bool(((y32.double() - op.y).abs() <= R.ln_delta(x, gm, bt, R.EPS)).all()), f"{name}: an fp32 LayerNorm further from fp64 than delta"
        off = (y32.to(torch.bfloat16).double() - op.yb).abs()
        assert bool((off <= op.unc).all()), f"{name}: a flip outside the uncertain set"
        flips += int((off > 0).sum())
    print(f"[decode-ref] h={h} {fam}: uncertain share {op.share:.4%}, flips inside it over three fp32 orders: {flips}")
    assert op.share <= R.UNCERTAIN_CAP


def test_a_harsh_row_is_rejected_not_accepted():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4, 1024, generator=g) * 0.1 + 100.0)
    gm, bt = R.ln_params(1024, g)
    with pytest.raises(AssertionError, match="uncertain share"):
        R.normalised(x, gm, bt, R.EPS)


# ------------------------------------------------------------------------------------------------------------------------------
# every case of the GPU list stays under the cap and lands where the list says (at the CU count it was written for)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.a_cases(), ids=lambda c: c.id)
def test_a_cases_under_the_cap_and_on_their_branch(case):
    form, mt, ks = R.a_form(case.M, case.h, case.lds)
    assert form == case.form and mt * ks <= 16
    assert case.n1 != 32 or (3 * case.h + case.n1) // 32 <= 200      # grid of the n1 = 32 shapes
    for fam in R.A_FAMILIES:
        qkv, a = R.a_reference(case, fam)            # asserts the cap and the GELU range
        assert qkv["op"].share <= R.UNCERTAIN_CAP and a["op"].share <= R.UNCERTAIN_CAP
        assert bool((qkv["bound"] > 0).all()) and bool(torch.isfinite(qkv["bound"]).all()) and bool(torch.isfinite(a["bound"]).all())


def test_a_cases_reach_every_direct_instantiation():
    direct = {(R.a_form(c.M, c.h, c.lds)[1:]) for c in R.a_cases() if c.form == "direct"}
    assert direct >= {(mt, ks) for ks in (1, 2, 3, 4) for mt in (1, 2, 3, 4)} | {(1, 8), (2, 8)}
    early = {mk for mk in direct if not R.late_gb(*mk)}
    assert early >= {(1, 1), (4, 1), (1, 2), (4, 2), (1, 3), (4, 3), (1, 4), (3, 4)} and (4, 4) not in early
    assert {R.a_form(c.M, c.h, c.lds)[1] for c in R.a_cases() if c.form == "lds"} == {1, 2}


@pytest.mark.parametrize("case", R.l_cases(), ids=lambda c: c.id)
def test_l_cases_under_the_cap_and_on_their_branch(case):
    assert R.linear_path(case.M, case.h, case.N, case.bias, R.CUS) == case.path
    if case.path == "head":
        assert ((case.N // 16) % R.CUS != 0) == (case.N != 64 * R.CUS)
    for fam in case.families:
        i = R.l_inputs(case, fam)
        assert R.normalised(i["x"], i["g"], i["b"], R.EPS).share <= R.UNCERTAIN_CAP


@pytest.mark.parametrize("case", R.out_cases(), ids=lambda c: c.id)
def test_out_cases_land_on_their_branch(case):
    form, P, ksl = R.out_plan(case.M, case.h, case.n1, R.CUS, case.lds)
    assert (form, P) == (case.form, case.P), (form, P, ksl)
    if "straddles" in case.note:
        assert R.straddles(case.h, P, ksl)
    if "falls back" in case.note:
        assert -(-((case.h + case.n1) // 32) // 16) == 17


# ------------------------------------------------------------------------------------------------------------------------------
# mutations
# ------------------------------------------------------------------------------------------------------------------------------
def _seen(mut, res):
    """the mutated value lies further than twice the bound from the reference somewhere"""
    return bool(((mut - res["ref"]).abs() > 2 * res["bound"]).any())


A_MUT = [R.ACase(M=13, h=256), R.ACase(M=29, h=1024, lds=True, form="lds"), R.ACase(M=29, h=2048)]


def _a(case, fam):
    assert case in R.a_cases()
    return R.a_inputs(case, fam), R.a_reference(case, fam)


@pytest.mark.parametrize("case", A_MUT, ids=lambda c: c.id)
@pytest.mark.parametrize("sign", [-1.0, 1.0], ids=["dropped", "duplicated"])
def test_one_k_fragment_dropped_or_duplicated_is_seen(case, sign):
    for fam in ("distinct", "census"):
        i, (qkv, a) = _a(case, fam)
        k0 = 8 * 37 % case.h
        for res, w, b, act in ((qkv, i["wqkv"], i["bqkv"], False), (a, i["w1"], i["bfc1"], True)):
            frag = res["op"].yb[:, k0:k0 + 8] @ w.double()[:, k0:k0 + 8].t()
            pre = res["op"].yb @ w.double().t() + b.double()
            mut = R.gelu(pre + sign * frag) if act else pre + sign * frag
            if fam == "distinct" or not act or bool((w[:, k0:k0 + 8] != 0).any()):
                assert _seen(mut, res), (fam, act)


@pytest.mark.parametrize("case", A_MUT, ids=lambda c: c.id)
def test_swapped_layernorm_parameters_are_seen(case):
    i, (qkv, a) = _a(case, "distinct")
    q2, a2 = R.ln_qkv_fc1(i["x"], i["g2"], i["b2"], i["g1"], i["b1"], R.EPS, i["wqkv"], i["bqkv"], i["w1"], i["bfc1"])
    assert _seen(q2["ref"], qkv) and _seen(a2["ref"], a)


@pytest.mark.parametrize("case", A_MUT, ids=lambda c: c.id)
def test_a_bias_shifted_by_four_columns_is_seen(case):
    i, (qkv, a) = _a(case, "distinct")
    assert _seen(qkv["ref"] - i["bqkv"].double() + torch.roll(i["bqkv"].double(), 4), qkv)
    pre = a["op"].yb @ i["w1"].double().t()
    assert _seen(R.gelu(pre + torch.roll(i["bfc1"].double(), 4)), a)
    lc = R.l_cases()[1]
    li, lr = R.l_inputs(lc, "distinct"), R.l_reference(lc, "distinct")
    assert _seen(lr["ref"] - li["bias"].double() + torch.roll(li["bias"].double(), 4), lr)


def _ln_with(x, g, b, mu, var, eps):
    return (x.double() - mu) / torch.sqrt(var + eps) * g.double() + b.double()


@pytest.mark.parametrize("case", A_MUT[1:], ids=lambda c: c.id)
def test_row_block_one_with_row_block_zeros_statistics_is_seen(case):
    for fam in ("distinct", "census"):
        i, (qkv, a) = _a(case, fam)
        mu, var = R.row_stats(i["x"])
        mu, var = mu.clone(), var.clone()
        n = case.M - 16
        mu[16:], var[16:] = mu[:n], var[:n]
        y1 = R.bf16_round(_ln_with(i["x"], i["g1"], i["b1"], mu, var, R.EPS))
        y2 = R.bf16_round(_ln_with(i["x"], i["g2"], i["b2"], mu, var, R.EPS))
        assert _seen(y1 @ i["wqkv"].double().t() + i["bqkv"].double(), qkv)
        assert _seen(R.gelu(y2 @ i["w1"].double().t() + i["bfc1"].double()), a)


@pytest.mark.parametrize("case", A_MUT, ids=lambda c: c.id)
def test_eps_left_out_is_seen_on_the_smallvar_row(case):
    i, (qkv, a) = _a(case, "edge")
    mu, var = R.row_stats(i["x"])
    y1 = R.bf16_round(_ln_with(i["x"], i["g1"], i["b1"], mu, var, 0.0))
    mut = y1 @ i["wqkv"].double().t() + i["bqkv"].double()
    far = (mut - qkv["ref"]).abs() > 2 * qkv["bound"]
    assert bool(far[1].any()), "the smallvar row does not show it"
    assert float(torch.sqrt((var[1] + R.EPS) / var[1])) > 1.03, "eps moves the smallvar row by several percent"


@pytest.mark.parametrize("case", A_MUT, ids=lambda c: c.id)
def test_unbiased_variance_is_seen_by_the_census(case):
    """(x - mu) / sigma moves by 1 / 2h of itself: under half a bf16 ulp of a product, but the census reads the operand bit for bit"""
    i, (qkv, a) = _a(case, "census")
    h = case.h
    mu, var = R.row_stats(i["x"])
    ym = _ln_with(i["x"], i["g1"], i["b1"], mu, var * h / (h - 1), R.EPS)
    d = R.ln_delta(i["x"], i["g1"], i["b1"], R.EPS)
    op = qkv["op"]
    sure_wrong = (op.unc == 0) & (R.bf16_round(ym - d) != op.yb) & (R.bf16_round(ym + d) != op.yb)
    assert int(sure_wrong.sum()) > 0
    got = R.bf16_round(ym)[:, R.census_k(3 * h, h)]
    wrong, _ = R.census_check(got, op, 3 * h)
    assert wrong > 0
    assert R.census_check(op.yb[:, R.census_k(3 * h, h)], op, 3 * h) == (0, 0.0)


OUT_MUT = [c for c in R.out_cases() if (c.h, c.n1, c.M) in ((256, 1792, 29), (768, 3712, 13), (1024, 7168, 9), (2048, 64, 29))]


def _out_mutations(case, i):
    """{name: x'} of the product mistakes, on the concatenated K axis [ao | act] . [wd | w2]"""
    _, P, ksl = R.out_plan(case.M, case.h, case.n1, R.CUS, case.lds)
    xc = torch.cat([i["ao"].double(), i["act"].double()], dim=1)
    wc = torch.cat([i["wd"].double(), i["w2"].double()], dim=1)
    base = i["x"].double() + i["bd"].double() + i["b2"].double()
    full = xc @ wc.t()
    muts = {}
    for p in sorted({0, P // 2, P - 1}):
        lo, hi = p * ksl * 32, min((p + 1) * ksl * 32, xc.shape[1])
        part = xc[:, lo:hi] @ wc[:, lo:hi].t()
        muts[f"slice {p} dropped"] = base + full - part
        muts[f"slice {p} twice"] = base + full + part
    muts["b_dense left out"] = base - i["bd"].double() + full
    for name in ("bd", "b2"):
        muts[f"{name} shifted by four columns"] = base - i[name].double() + torch.roll(i[name].double(), 4) + full
    kh = case.h
    seam = xc[:, kh - 32:kh] @ wc[:, kh - 32:kh].t() - xc[:, kh:kh + 32] @ wc[:, kh:kh + 32].t()
    muts["seam one k-step late"] = base + full + seam      # the last dense step read again in place of the first fc2 step
    return muts


@pytest.mark.parametrize("case", OUT_MUT, ids=lambda c: c.id)
def test_out_mutations_are_seen(case):
    assert len(OUT_MUT) == 4
    i, res = R.out_inputs(case, "random"), R.out_reference(case, "random")
    for name, mut in _out_mutations(case, i).items():
        assert _seen(mut, res), name
    i, res = R.out_inputs(case, "integers"), R.out_reference(case, "integers")
    assert float(res["A"].max()) + 30 < 2 ** 24 and torch.equal(res["ref"], res["ref"].float().double())
    for name, mut in _out_mutations(case, i).items():
        assert not torch.equal(mut, res["ref"]), name
