"""The LwF head-loss kernels (csrc/kd.hip: mafed_ce_kd_fwd / mafed_ce_kd_bwd) through the C-ABI wrappers against the float64
restatement of tests/kd_ref.py, which is fed the same, already-rounded inputs upcast to float64.

Bounds (per element, against float64):
  * out3 = (loss, CE, KD) and the three saved log-sum-exps: 1e-5 * max(1, max|logit| / tau) -- the bound of ``token_logprob``, scaled
    to the largest argument an exponential sees in the tau domain
  * fp32 dlogits: 1e-6 |g_b| + 1e-5 |value|;  bf16 dlogits: one bf16 rounding of the float64 value, 2^-8 |value| + 1e-7 |g_b| (the only
    bf16 step is the final store)
Shapes: V = 512 (half the threads of a row's block idle), V = 1028 (no multiple of the 1024-element stride of the 4-element loads; bf16
rows not 16-byte aligned -> the 8-byte load path), V = 50304 (the production vocabulary; 16-byte bf16 loads, many trips).  Labels: a fully
labelled sample, one with a single labelled row whose label sits in the row's last 4-element group, one with none.
"""
import itertools
import math

import pytest
import torch

from tests.kd_ref import kd_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(2, 3, 512), (3, 5, 1028), (2, 4, 50304)]
TAUS = (0.5, 1.0, 2.0)
LAMS = (0.0, 1.0, 0.3)
GLOSS = 1.7
KINDS = ("full", "one", "none")


def _labels(B, T, V, first, seed):
    """Sample b is of kind KINDS[(first + b) % 3]: every row labelled (one of them with V - 1), one labelled row (label V - 2: the last
    4-element group of the row), or no label."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.full((B, T), -100, dtype=torch.int64)
    for b in range(B):
        kind = KINDS[(first + b) % 3]
        if kind == "full":
            labels[b, 1:] = torch.randint(0, V, (T - 1,), generator=g)
            labels[b, 1] = V - 1
            labels[b, 0] = 5   # (predicted by nothing: must not matter)
        elif kind == "one":
            labels[b, T - 1] = V - 2
    return labels


def _logits(B, T, V, recipe, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    s, t = torch.randn(B, T, V, generator=g), torch.randn(B, T, V, generator=g)
    if recipe == "hard":
        # scale 30 and one +80 outlier per row, at different columns of student and teacher: at tau = 0.5 an exponential that is not
        # max-subtracted overflows (160 > 88.7)
        s, t = s * 30.0, t * 30.0
        cs = torch.randint(0, V, (B, T), generator=g)
        ct = (cs + 1 + torch.randint(0, V - 1, (B, T), generator=g)) % V
        s.scatter_add_(-1, cs.unsqueeze(-1), torch.full((B, T, 1), 80.0))
        t.scatter_add_(-1, ct.unsqueeze(-1), torch.full((B, T, 1), 80.0))
    return s.to(dtype), t.to(dtype)


_CASES = {}


def _case(shape, dtype, recipe, first):
    """(student, teacher, labels) on the GPU + {(tau, lam): kd_ref} -- built once, shared, never modified."""
    key = (shape, dtype, recipe, first)
    if key not in _CASES:
        B, T, V = shape
        seed = 1000 * SHAPES.index(shape) + 10 * first + (1 if recipe == "hard" else 0)
        s, t = _logits(B, T, V, recipe, dtype, seed)
        labels = _labels(B, T, V, first, seed + 7)
        refs = {(tau, lam): kd_ref(s, t, labels, tau, lam, gloss=GLOSS) for tau, lam in itertools.product(TAUS, LAMS)}
        _CASES[key] = (s.to(DEV), t.to(DEV), labels.to(DEV), refs, float(max(s.float().abs().max(), t.float().abs().max())))
    return _CASES[key]


def _check_dlogits(d, ref, dtype, what):
    got = d.double().cpu()
    want, g = ref["dlogits"], ref["g"].abs().view(-1, 1, 1)
    bound = (1e-6 * g + 1e-5 * want.abs()) if dtype == torch.float32 else (2.0 ** -8 * want.abs() + 1e-7 * g)
    err = (got - want).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"[kd] {what}: dlogits max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert torch.isfinite(got).all(), what
    assert bool((err <= bound).all()), f"{what}: dlogits exceed the bound by up to {worst:.3f} x"
    assert float(got[~ref["mask"]].abs().max() if (~ref["mask"]).any() else 0.0) == 0.0, f"{what}: unlabelled rows must be zero"


@pytest.mark.parametrize("first", [0, 2])
@pytest.mark.parametrize("recipe", ["normal", "hard"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_ce_kd_kernels_against_fp64(shape, dtype, recipe, first):
    from mafed_amd import ops
    s, t, labels, refs, amax = _case(shape, dtype, recipe, first)
    gl = torch.tensor([GLOSS], device=DEV)
    for (tau, lam), ref in refs.items():
        what = f"{shape} {str(dtype)[6:]} {recipe} first={KINDS[first]} tau={tau} lam={lam}"
        out3, lse3 = ops.ce_kd_fwd(s, t, labels, tau, lam)
        d = ops.ce_kd_bwd(s, t, labels, lse3, tau, lam, gl)
        torch.cuda.synchronize()
        bound = 1e-5 * max(1.0, amax / tau)
        e_out = float((out3.double().cpu() - ref["out3"]).abs().max())
        e_lse = float((lse3.double().cpu() - ref["lse3"]).abs().max())
        print(f"[kd] {what}: out3 {[float(x) for x in out3]} err {e_out:.3e}, lse3 err {e_lse:.3e} (bound {bound:.3e})")
        assert torch.isfinite(out3).all() and torch.isfinite(lse3).all(), what
        assert e_out <= bound, f"{what}: out3 off by {e_out:.3e} > {bound:.3e}"
        assert e_lse <= bound, f"{what}: lse3 off by {e_lse:.3e} > {bound:.3e}"
        if tau == 1.0:
            assert torch.equal(lse3[0], lse3[1]), f"{what}: tau == 1 must give the two student LSEs the same bits"
        _check_dlogits(d, ref, dtype, what)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_identical_teacher_and_lambda_zero_reduce_to_the_cross_entropy(dtype):
    """teacher == student: KD == 0.0 exactly, loss == CE, the gradient is the cross-entropy kernel's; lambda = 0 likewise for any teacher.
    Against ops.ce_fwd / ops.ce_bwd on N(0, 1) logits: the loss within 1e-6 max(1, |CE|), fp32 dlogits within 1e-6 |g_b| (the two kernels
    differ in their exponential and in the last bit of the saved log-sum-exp); in bf16 the two fp32 values may in addition fall on either
    side of a rounding boundary of the store: one bf16 ulp, 2^-7 |value|."""
    from mafed_amd import ops
    shape = (3, 5, 1028)
    s, t, labels, refs, _ = _case(shape, dtype, "normal", 0)
    gl = torch.tensor([GLOSS], device=DEV)
    ce, lse = ops.ce_fwd(s, labels)
    dce = ops.ce_bwd(s, labels, lse, gl)
    g = refs[(1.0, 1.0)]["g"].abs().view(-1, 1, 1).to(DEV)

    def same_as_ce(out3, d, what):
        assert abs(float(out3[1]) - float(ce)) <= 1e-6 * max(1.0, abs(float(ce))), (what, float(out3[1]), float(ce))
        assert abs(float(out3[0]) - float(ce)) <= 1e-6 * max(1.0, abs(float(ce))), (what, float(out3[0]), float(ce))
        bound = 1e-6 * g + (0.0 if dtype == torch.float32 else 2.0 ** -7) * dce.double().abs()
        err = (d.double() - dce.double()).abs()
        print(f"[kd] {what}: max |dlogits - ce_bwd| {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), what

    for tau in TAUS:
        out3, lse3 = ops.ce_kd_fwd(s, s.clone(), labels, tau, 1.0)
        d = ops.ce_kd_bwd(s, s.clone(), labels, lse3, tau, 1.0, gl)
        torch.cuda.synchronize()
        assert float(out3[2]) == 0.0, f"tau {tau}: KD of identical logits is {float(out3[2])!r}, not exactly 0"
        assert float(out3[0]) == float(out3[1])
        assert torch.equal(lse3[1], lse3[2])
        same_as_ce(out3, d, f"{str(dtype)[6:]} teacher == student, tau {tau}")
        out3, lse3 = ops.ce_kd_fwd(s, s, labels, tau, 1.0)   # the same buffer
        assert float(out3[2]) == 0.0 and float(out3[0]) == float(out3[1])
        out3, lse3 = ops.ce_kd_fwd(s, t, labels, tau, 0.0)
        d = ops.ce_kd_bwd(s, t, labels, lse3, tau, 0.0, gl)
        torch.cuda.synchronize()
        assert float(out3[2]) > 0.0
        same_as_ce(out3, d, f"{str(dtype)[6:]} lambda 0, tau {tau}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unlabelled_sample_repeatability_and_poison(dtype):
    from mafed_amd import ops
    shape = (3, 5, 1028)
    s, t, labels, refs, _ = _case(shape, dtype, "hard", 0)
    gl = torch.tensor([GLOSS], device=DEV)
    tau, lam = 0.5, 1.0
    out3, lse3 = ops.ce_kd_fwd(s, t, labels, tau, lam)
    d = ops.ce_kd_bwd(s, t, labels, lse3, tau, lam, gl)
    # sample 2 has no label: nothing from it in the loss (the first two samples alone, averaged over the same B, give the same bits)
    assert float(d[2].abs().max()) == 0.0 and float(lse3[:, 2].abs().max()) == 0.0
    s2, t2 = s.clone(), t.clone()
    s2[2], t2[2] = 0.0, 123.0
    assert torch.equal(ops.ce_kd_fwd(s2, t2, labels, tau, lam)[0], out3)
    # every label ignored: 0, not NaN
    none = torch.full_like(labels, -100)
    o0, l0 = ops.ce_kd_fwd(s, t, none, tau, lam)
    d0 = ops.ce_kd_bwd(s, t, none, l0, tau, lam, gl)
    assert float(o0.abs().max()) == 0.0 and float(d0.abs().max()) == 0.0
    # the same bits on every call
    out3b, lse3b = ops.ce_kd_fwd(s, t, labels, tau, lam)
    db = ops.ce_kd_bwd(s, t, labels, lse3b, tau, lam, gl)
    assert torch.equal(out3, out3b) and torch.equal(lse3, lse3b) and torch.equal(d, db)
    # a raised poison flag turns the loss, and only the loss, into NaN
    for flag, bad in ((0, False), (1, True)):
        o, _ = ops.ce_kd_fwd(s, t, labels, tau, lam, poison=torch.tensor([flag], dtype=torch.int32, device=DEV))
        assert math.isnan(float(o[0])) == bad and torch.equal(o[1:], out3[1:])
        if not bad:
            assert torch.equal(o, out3)


def test_profiler_tags_and_byte_counts():
    """The two launches carry their own tags; algorithmic bytes: forward 2 rows V elt, backward 3 rows V elt."""
    from mafed_amd import ops
    from mafed_amd.profiler import KernelProfile
    shape = (3, 5, 1028)
    B, T, V = shape
    gl = torch.tensor([GLOSS], device=DEV)
    for dtype, elt in ((torch.float32, 4), (torch.bfloat16, 2)):
        s, t, labels, _, _ = _case(shape, dtype, "normal", 0)
        with KernelProfile() as prof:
            _, lse3 = ops.ce_kd_fwd(s, t, labels, 2.0, 1.0)
            ops.ce_kd_bwd(s, t, labels, lse3, 2.0, 1.0, gl)
        recs = [(tag, work) for tag, work, ms in prof.records() if ms >= 0]
        assert recs == [("ce_kd_fwd", 2.0 * B * T * V * elt), ("small", 0.0), ("ce_kd_bwd", 3.0 * B * T * V * elt)], recs


def test_refusals():
    from mafed_amd import _lib, ops
    s = torch.randn(2, 3, 512, device=DEV)
    labels = torch.zeros(2, 3, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.MafedHipError):
        ops.ce_kd_fwd(s, s, labels, 0.0, 1.0)          # tau must be positive
    with pytest.raises(_lib.MafedHipError):
        ops.ce_kd_fwd(s[..., :510].contiguous(), s[..., :510].contiguous(), labels, 1.0, 1.0)   # V % 4
    with pytest.raises(ValueError):
        ops.ce_kd_fwd(s, s.to(torch.bfloat16), labels, 1.0, 1.0)
