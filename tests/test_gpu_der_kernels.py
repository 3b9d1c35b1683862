"""The DER++ head-loss kernels (csrc/der.hip: mafed_ce_mse_fwd / mafed_ce_mse_bwd) through the C-ABI wrappers against the float64
restatement of tests/der_ref.py, which is fed the same, already-rounded inputs upcast to float64.

Bounds (per element, against float64):
  * CE (out3[1]) and the saved log-sum-exp: 1e-5 * max(1, max|logit|) -- the bound of tests/test_gpu_kd.py at tau = 1
  * MSE (out3[2]): 1e-5 of the float64 value.  The fp32 sum is of non-negative terms, at most 50 sequential adds in a thread (V = 50304
    in steps of 1024) and a 14-level tree behind them: a relative error of at most about 64 * 2^-24 = 4e-6
  * the loss (out3[0] = beta CE + alpha MSE): beta times the CE bound + alpha times the MSE bound + 2^-22 (beta |CE| + alpha |MSE|) for
    the two roundings of the combination
  * fp32 dlogits: 1e-6 |g_b| m + 1e-5 |value|;  bf16 dlogits: one bf16 rounding of the float64 value, 2^-8 |value| + 1e-7 |g_b| m;
    m = max(1, 2 alpha max|s - z| / V) -- the bounds of tests/test_gpu_kd.py, the absolute floor scaled to the largest squared-distance term
Shapes: V = 512 (half the threads of a row's block idle), V = 1028 (no multiple of the 1024-element stride; bf16 rows that are only
8-byte aligned), V = 50304 (the production vocabulary, many trips; two samples of four rows).  The store is [7, 3, V]; ``mem_index`` is
unordered and repeats a sample.  Samples: every row a store can hold labelled, one labelled row sitting last, labelled / unlabelled /
labelled (rank != offset), no label.
"""
import math

import pytest
import torch

from tests.der_ref import der_ref, rank_map

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(3, 5, 512), (3, 5, 1028), (2, 4, 50304)]
N_MEM, A = 7, 3
MEM_INDEX = {3: [5, 0, 5], 2: [5, 0]}
COEFS = ((0.5, 1.0), (1.0, 0.0), (0.0, 1.0), (0.3, 0.7))
GLOSS = 1.7
KINDS = ("full", "one", "gap", "none")


def _labels(B, T, V, first, seed):
    """Sample b is of kind KINDS[(first + b) % 4]: the last min(T - 1, A) rows labelled (every row when T - 1 <= A; one label is V - 1),
    one labelled row sitting last (label V - 2: the last 4-element group of the row), rows 0 and 2 labelled with row 1 between them
    (the second labelled row has rank 1 at offset 2), or no label."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.full((B, T), -100, dtype=torch.int64)
    for b in range(B):
        kind = KINDS[(first + b) % 4]
        if kind == "full":
            n = min(T - 1, A)
            labels[b, T - n:] = torch.randint(0, V, (n,), generator=g)
            labels[b, T - n] = V - 1
            labels[b, 0] = 5 if n == T - 1 else -100   # (predicted by nothing: must not matter)
        elif kind == "one":
            labels[b, T - 1] = V - 2
        elif kind == "gap":
            labels[b, 1], labels[b, 3] = 7, V - 3
    return labels


def _logits(shape, recipe, dtype, g):
    x = torch.randn(*shape, generator=g)
    if recipe == "hard":   # scale 30 and one +80 outlier per row (the "hard" recipe of tests/test_gpu_kd.py)
        x = x * 30.0
        c = torch.randint(0, shape[-1], shape[:-1], generator=g)
        x.scatter_add_(-1, c.unsqueeze(-1), torch.full(shape[:-1] + (1,), 80.0))
    return x.to(dtype)


_CASES = {}


def _case(shape, dtype, recipe, first):
    """(student, store, mem_index, labels) on the GPU + {(alpha, beta): der_ref} -- built once, shared, never modified."""
    key = (shape, dtype, recipe, first)
    if key not in _CASES:
        B, T, V = shape
        seed = 1000 * SHAPES.index(shape) + 10 * first + (1 if recipe == "hard" else 0)
        g = torch.Generator().manual_seed(seed)
        s = _logits((B, T, V), recipe, dtype, g)
        store = _logits((N_MEM, A, V), recipe, dtype, g)
        mi = torch.tensor(MEM_INDEX[B], dtype=torch.int64)
        labels = _labels(B, T, V, first, seed + 7)
        refs = {ab: der_ref(s, store, mi, labels, ab[0], ab[1], gloss=GLOSS) for ab in COEFS}
        _CASES[key] = (s.to(DEV), store.to(DEV), mi.to(DEV), labels.to(DEV), refs, float(s.float().abs().max()))
    return _CASES[key]


def _check_dlogits(d, ref, dtype, alpha, V, what):
    got = d.double().cpu()
    want = ref["dlogits"]
    g = ref["g"].abs().view(-1, 1, 1) * max(1.0, 2.0 * alpha * ref["dmax"] / V)
    bound = (1e-6 * g + 1e-5 * want.abs()) if dtype == torch.float32 else (2.0 ** -8 * want.abs() + 1e-7 * g)
    err = (got - want).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"[der] {what}: dlogits max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert torch.isfinite(got).all(), what
    assert bool((err <= bound).all()), f"{what}: dlogits exceed the bound by up to {worst:.3f} x"
    assert float(got[~ref["mask"]].abs().max() if (~ref["mask"]).any() else 0.0) == 0.0, f"{what}: unlabelled rows must be zero"


@pytest.mark.parametrize("first", [0, 2])
@pytest.mark.parametrize("recipe", ["normal", "hard"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_ce_mse_kernels_against_fp64(shape, dtype, recipe, first):
    from mafed_amd import ops
    s, store, mi, labels, refs, amax = _case(shape, dtype, recipe, first)
    gl = torch.tensor([GLOSS], device=DEV)
    V = shape[2]
    for (alpha, beta), ref in refs.items():
        what = f"{shape} {str(dtype)[6:]} {recipe} first={KINDS[first]} alpha={alpha} beta={beta}"
        out3, lse = ops.ce_mse_fwd(s, store, mi, labels, alpha, beta)
        d = ops.ce_mse_bwd(s, store, mi, labels, lse, alpha, beta, gl)
        torch.cuda.synchronize()
        want = ref["out3"]
        b_ce = 1e-5 * max(1.0, amax)
        b_mse = 1e-5 * float(want[2])
        b_loss = beta * b_ce + alpha * b_mse + 2.0 ** -22 * (beta * abs(float(want[1])) + alpha * float(want[2]))
        e = (out3.double().cpu() - want).abs()
        e_lse = float((lse.double().cpu() - ref["lse"]).abs().max())
        print(f"[der] {what}: out3 {[float(x) for x in out3]} err {[float(x) for x in e]} (bounds {b_loss:.3e}, {b_ce:.3e}, {b_mse:.3e}), "
              f"lse err {e_lse:.3e}")
        assert torch.isfinite(out3).all() and torch.isfinite(lse).all(), what
        assert float(want[2]) > 0.0
        assert float(e[1]) <= b_ce, f"{what}: CE off by {float(e[1]):.3e} > {b_ce:.3e}"
        assert float(e[2]) <= b_mse, f"{what}: MSE off by {float(e[2]):.3e} > {b_mse:.3e}"
        assert float(e[0]) <= b_loss, f"{what}: loss off by {float(e[0]):.3e} > {b_loss:.3e}"
        assert e_lse <= b_ce, f"{what}: lse off by {e_lse:.3e} > {b_ce:.3e}"
        _check_dlogits(d, ref, dtype, alpha, V, what)


def _store_of_student(s, labels, mem_index, like):
    """A store whose row [m_b, j] is the student's own row (b, t) for every labelled row; random elsewhere.  ``mem_index`` without a
    repeat."""
    store = like.clone()
    for b, t, j in rank_map(labels):
        store[int(mem_index[b]), j] = s[b, t]
    return store


@pytest.mark.parametrize("shape", [(3, 5, 1028), (2, 4, 50304)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stored_rows_equal_to_the_student_and_alpha_zero_give_the_cross_entropy_bits(shape, dtype):
    """store[m_b, j] == s bit for bit: MSE == 0.0 exactly and, with beta = 1, loss == CE; loss, the log-sum-exp of the labelled rows and
    dlogits are those of ops.ce_fwd / ops.ce_bwd bit for bit.  (ops.ce_fwd also returns the log-sum-exp of unlabelled rows in front of
    the last position; the DER kernel does not read those rows and leaves 0.)  alpha = 0 with any store: the same bits."""
    from mafed_amd import ops
    B = shape[0]
    for first in (0, 2):
        s, store, _, labels, refs, _ = _case(shape, dtype, "normal", first)
        mask = refs[COEFS[0]]["mask"].to(DEV)
        gl = torch.tensor([GLOSS], device=DEV)
        ce, lse_ce = ops.ce_fwd(s, labels)
        dce = ops.ce_bwd(s, labels, lse_ce, gl)
        mi = torch.tensor([6, 0, 3][:B], dtype=torch.int64, device=DEV)
        same = _store_of_student(s, labels.cpu(), mi.cpu(), store)
        for st, alpha in ((same, 0.5), (same, 1.0), (store, 0.0)):
            out3, lse = ops.ce_mse_fwd(s, st, mi, labels, alpha, 1.0)
            d = ops.ce_mse_bwd(s, st, mi, labels, lse, alpha, 1.0, gl)
            torch.cuda.synchronize()
            what = f"{shape} {str(dtype)[6:]} first={KINDS[first]} alpha={alpha}"
            if st is same:
                assert float(out3[2]) == 0.0, f"{what}: MSE of identical rows is {float(out3[2])!r}, not exactly 0"
            else:
                assert float(out3[2]) > 0.0
            assert float(out3[0]) == float(out3[1]) == float(ce), (what, out3, float(ce))
            assert torch.equal(lse[mask], lse_ce[mask]) and float(lse[~mask].abs().max()) == 0.0, what
            assert torch.equal(d, dce), f"{what}: max |dlogits - ce_bwd| {float((d.float() - dce.float()).abs().max()):.3e}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_that_are_not_read_repeatability_and_poison(dtype):
    from mafed_amd import ops
    shape = (3, 5, 1028)
    s, store, mi, labels, refs, _ = _case(shape, dtype, "hard", 2)   # samples: gap, none, full; mem_index [5, 0, 5]
    gl = torch.tensor([GLOSS], device=DEV)
    alpha, beta = 0.5, 1.0
    out3, lse = ops.ce_mse_fwd(s, store, mi, labels, alpha, beta)
    d = ops.ce_mse_bwd(s, store, mi, labels, lse, alpha, beta, gl)
    assert float(d[1].abs().max()) == 0.0 and float(lse[1].abs().max()) == 0.0
    # the sample without a label: neither its student rows nor its store rows are read
    s2, st2 = s.clone(), store.clone()
    s2[1], st2[0] = float("nan"), float("nan")
    o2, l2 = ops.ce_mse_fwd(s2, st2, mi, labels, alpha, beta)
    d2 = ops.ce_mse_bwd(s2, st2, mi, labels, l2, alpha, beta, gl)
    assert torch.equal(o2, out3) and torch.equal(l2, lse) and torch.equal(d2, d)
    # store rows no batch row maps to: NaN there changes nothing (and unlabelled rows of labelled samples are not read either)
    used = {(int(mi[b]), j) for b, t, j in rank_map(labels.cpu())}
    st3, s3 = store.clone(), s.clone()
    for m in range(N_MEM):
        for j in range(A):
            if (m, j) not in used:
                st3[m, j] = float("nan")
    s3[~refs[(alpha, beta)]["mask"].to(DEV)] = float("nan")
    assert used == {(5, 0), (5, 1), (5, 2)} and float(torch.isnan(st3).float().mean()) > 0.5
    o3, l3 = ops.ce_mse_fwd(s3, st3, mi, labels, alpha, beta)
    d3 = ops.ce_mse_bwd(s3, st3, mi, labels, l3, alpha, beta, gl)
    assert torch.equal(o3, out3) and torch.equal(l3, lse) and torch.equal(d3, d)
    # every label ignored: 0, not NaN
    none = torch.full_like(labels, -100)
    o0, l0 = ops.ce_mse_fwd(s, store, mi, none, alpha, beta)
    d0 = ops.ce_mse_bwd(s, store, mi, none, l0, alpha, beta, gl)
    assert float(o0.abs().max()) == 0.0 and float(d0.abs().max()) == 0.0
    # the same bits on every call
    out3b, lseb = ops.ce_mse_fwd(s, store, mi, labels, alpha, beta)
    db = ops.ce_mse_bwd(s, store, mi, labels, lseb, alpha, beta, gl)
    assert torch.equal(out3, out3b) and torch.equal(lse, lseb) and torch.equal(d, db)
    # a raised poison flag turns the loss, and only the loss, into NaN
    for flag, bad in ((0, False), (1, True)):
        o, _ = ops.ce_mse_fwd(s, store, mi, labels, alpha, beta, poison=torch.tensor([flag], dtype=torch.int32, device=DEV))
        assert math.isnan(float(o[0])) == bad and torch.equal(o[1:], out3[1:])
        if not bad:
            assert torch.equal(o, out3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_row_without_a_stored_row_answers_with_nan(dtype):
    """mem_index == n_mem, mem_index == -1, or a sample with A + 1 labelled rows: refused by value inside the kernel (anchor_row returns
    null before an address into the store is formed) -- NaN in the loss, in MSE and in that row's gradient; CE and the other samples'
    gradients stay as they were."""
    from mafed_amd import ops
    shape = (3, 5, 512)
    s, store, mi, labels, refs, _ = _case(shape, dtype, "normal", 0)   # samples: full (3 rows), one, gap
    gl = torch.tensor([GLOSS], device=DEV)
    alpha, beta = 0.5, 1.0
    out3, lse = ops.ce_mse_fwd(s, store, mi, labels, alpha, beta)
    d = ops.ce_mse_bwd(s, store, mi, labels, lse, alpha, beta, gl)
    four = labels.clone()
    four[0, 1:] = torch.tensor([3, 4, 5, 6], device=DEV)   # A + 1 labelled rows
    for what, mi2, lab2, bad_b in (("mem_index = n_mem", torch.tensor([5, N_MEM, 5], device=DEV), labels, 1),
                                   ("mem_index = -1", torch.tensor([5, 0, -1], device=DEV), labels, 2),
                                   ("A + 1 labelled rows", mi, four, 0)):
        o, l = ops.ce_mse_fwd(s, store, mi2, lab2, alpha, beta)
        dd = ops.ce_mse_bwd(s, store, mi2, lab2, l, alpha, beta, gl)
        torch.cuda.synchronize()
        assert math.isnan(float(o[0])) and math.isnan(float(o[2])) and math.isfinite(float(o[1])), (what, o)
        assert torch.isfinite(l).all(), what
        bad = torch.isnan(dd.float()).any(dim=-1)
        assert bool(bad[bad_b].any()) and not bool(bad[[b for b in range(3) if b != bad_b]].any()), (what, bad)
        if lab2 is labels:
            assert float(o[1]) == float(out3[1])
            for b in range(3):
                if b != bad_b:
                    assert torch.equal(dd[b], d[b]), what
        else:
            assert bad[0].tolist() == [False, False, False, True, False], bad   # only the row of rank 3 has no stored row


def test_profiler_tags_and_byte_counts():
    """The two launches carry their own tags; algorithmic bytes: forward 2 rows V elt, backward 3 rows V elt."""
    from mafed_amd import ops
    from mafed_amd.profiler import KernelProfile
    shape = (3, 5, 1028)
    B, T, V = shape
    gl = torch.tensor([GLOSS], device=DEV)
    for dtype, elt in ((torch.float32, 4), (torch.bfloat16, 2)):
        s, store, mi, labels, _, _ = _case(shape, dtype, "normal", 0)
        with KernelProfile() as prof:
            _, lse = ops.ce_mse_fwd(s, store, mi, labels, 0.5, 1.0)
            ops.ce_mse_bwd(s, store, mi, labels, lse, 0.5, 1.0, gl)
        recs = [(tag, work) for tag, work, ms in prof.records() if ms >= 0]
        assert recs == [("ce_mse_fwd", 2.0 * B * T * V * elt), ("small", 0.0), ("ce_mse_bwd", 3.0 * B * T * V * elt)], recs


def test_refusals():
    from mafed_amd import _lib, ops
    B, T, V = 2, 3, 512
    s = torch.randn(B, T, V, device=DEV)
    store = torch.randn(N_MEM, A, V, device=DEV)
    labels = torch.zeros(B, T, dtype=torch.int64, device=DEV)
    mi = torch.zeros(B, dtype=torch.int64, device=DEV)
    gl = torch.ones(1, device=DEV)
    out3, lse = ops.ce_mse_fwd(s, store, mi, labels, 0.5, 1.0)
    # the wrappers: dtype, V, mem_index
    with pytest.raises(ValueError):
        ops.ce_mse_fwd(s, store.to(torch.bfloat16), mi, labels, 0.5, 1.0)
    with pytest.raises(ValueError):
        ops.ce_mse_fwd(s, store[..., :256].contiguous(), mi, labels, 0.5, 1.0)
    with pytest.raises(ValueError):
        ops.ce_mse_fwd(s, store, mi.to(torch.int32), labels, 0.5, 1.0)
    with pytest.raises(ValueError):
        ops.ce_mse_fwd(s, store, mi[:1], labels, 0.5, 1.0)
    with pytest.raises(_lib.MafedHipError):
        ops.ce_mse_fwd(s[..., :510].contiguous(), store[..., :510].contiguous(), mi, labels, 0.5, 1.0)   # V % 4
    with pytest.raises(_lib.MafedHipError):
        ops.ce_mse_fwd(s, store, mi, labels, float("inf"), 1.0)
    # the entry points: null, A <= 0, n_mem <= 0, misalignment -- refused before a launch
    lib = _lib.load()
    row = torch.empty(3, B, T, device=DEV)
    p = lambda t: t.data_ptr()

    def fwd(student=p(s), st=p(store), dt=ops.F32, mem=p(mi), n_mem=N_MEM, a=A, v=V):
        return lib.mafed_ce_mse_fwd(student, st, dt, p(labels), mem, B, T, v, n_mem, a, 0.5, 1.0, p(row[0]), p(row[1]), p(row[2]), p(out3), 0, 0)

    def bwd(student=p(s), st=p(store), dt=ops.F32, a=A, out=None):
        out = torch.empty_like(s) if out is None else out
        return lib.mafed_ce_mse_bwd(student, st, dt, p(labels), p(mi), p(lse), B, T, V, N_MEM, a, 0.5, 1.0, p(gl), out if isinstance(out, int) else p(out), 0)

    torch.cuda.synchronize()
    assert fwd() == 0 and bwd() == 0
    for rc in (fwd(st=0), fwd(mem=0), fwd(a=0), fwd(a=-1), fwd(n_mem=0), fwd(v=510), fwd(student=p(s) + 4), fwd(st=p(store) + 8),
               fwd(dt=ops.BF16, student=p(s) + 2), fwd(dt=ops.BF16, st=p(store) + 4),
               bwd(st=0), bwd(a=0), bwd(out=0), bwd(st=p(store) + 8), bwd(out=p(s) + 4), bwd(dt=ops.BF16, st=p(store) + 2)):
        assert rc != 0
    torch.cuda.synchronize()
