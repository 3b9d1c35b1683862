"""GEM's three entry points (csrc/gem.hip) against float64 numpy (tests/gem_ref.py): the Gram over K + 1 flat buffers, the exact
on-device solve on crafted Gram matrices, the K-term AXPY with its norm hand-over, and the argument checks."""
import numpy as np
import pytest
import torch

from tests import gem_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24

# 0: empty; 1, 3: tail only; 4: one vector; 1023: less than one block; 4 * 1024 + 1: several blocks and a tail behind full vectors
SIZES = [0, 1, 3, 4, 1023, 4 * 1024 + 1]
KS = [1, 2, 3, 8]            # 1 .. 3: two vectors per trip; 8: one vector per trip, 45 accumulators
BIG = 3 * 2 ** 21 + 5        # several vectors per thread through the grid-stride loop, and a tail
GRID = [(n, K) for n in SIZES for K in KS] + [(BIG, 1), (BIG, 8)]
TAIL = 64.0                  # planted in the last element of every buffer: 4096 in every Gram entry, far above the bounds below

_INPUTS = {}


def _inputs(n, K):
    """(g, refs) fp32 on the device and their float64 numpy copies; built once per case and left unchanged.  g[2] = -0.0; the last
    element of every buffer (the n % 4 tail where there is one) carries TAIL."""
    key = (n, K)
    if key not in _INPUTS:
        gen = torch.Generator().manual_seed(2000 + n % 997 + 13 * K)
        xs = [torch.randn(n, generator=gen) for _ in range(K + 1)]
        if n > 2:
            xs[0][2] = -0.0
        if n > 4:
            for x in xs:
                x[n - 1] = TAIL
        _INPUTS[key] = ([x.to(DEV) for x in xs], [x.double().numpy() for x in xs])
    (g, *refs), (g64, *refs64) = _INPUTS[key]
    return g, refs, g64, refs64


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def gram_bound_factor(n):
    """c of the bound c 2^-24 sum|x_a x_b| on a Gram entry, from the grid rule: every thread adds one 4-term dot per vector it owns
    into its accumulator -- ceil(n4 / threads) dependent additions, one more for the tail --, the 4-term dot itself rounds three times
    along its longest path (product, inner sum, outer sum), the block tree adds 6 levels of wave shuffles and 4 wave sums.  The fold of
    the per-block partials is in double.  (First order; c 2^-24 <= 2e-6 here, so the second-order term is below 1e-11.)"""
    from mafed_amd import ops
    threads = ops.gem_blocks(n) * 256
    n4 = n // 4
    return -(-n4 // threads) + 1 + 3 + 6 + 4


@pytest.mark.parametrize("n,K", GRID)
def test_gem_gram_vs_fp64(n, K):
    from mafed_amd import ops
    g, refs, g64, refs64 = _inputs(n, K)
    want, sabs = (G.gem_gram(g64, refs64) if n else (np.zeros((K + 1, K + 1)),) * 2)
    a = ops.gem_gram(g, refs)
    b = ops.gem_gram(g, refs, torch.full((K + 1, K + 1), -7.0, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert a.dtype == torch.float64 and a.shape == (K + 1, K + 1)
    assert torch.equal(_bits(a), _bits(b)), "not the same bits run to run"
    assert torch.equal(_bits(a), _bits(a.t())), "not symmetric to the bit"
    got = a.cpu().numpy()
    c = gram_bound_factor(n)
    err, bound = np.abs(got - want), c * U24 * sabs
    print(f"[gem] gram n {n} K {K}: c {c}, worst err / bound {float((err / np.where(bound > 0, bound, 1)).max()):.3f}, "
          f"worst err / sum|x x| {float((err / np.where(sabs > 0, sabs, 1)).max()):.3e}")
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"
    if n == 0:
        assert not got.any()
    if n > 4:
        # a Gram without the last element (in the n % 4 tail at these sizes) would miss every bound: the tail path carries weight
        assert n % 4 and bool((np.abs(want - TAIL * TAIL - got) > bound).all())


# ---- solve ----------------------------------------------------------------------------------------------------------------------
def _solve(gram, margin, eps):
    from mafed_amd import ops
    K = gram.shape[0] - 1
    st = ops.gem_solve(torch.as_tensor(gram, dtype=torch.float64).contiguous().to(DEV), K, margin, eps,
                       torch.full((12,), -7.0, device=DEV))
    return st.cpu().numpy()


def _gram_of(P, q, g0=None):
    K = len(q)
    gram = np.zeros((K + 1, K + 1))
    gram[1:, 1:], gram[0, 1:], gram[1:, 0] = P, q, q
    gram[0, 0] = 1.0 + float(np.abs(q).sum()) if g0 is None else g0
    return gram


def _check_against_oracle(st, gram, margin, eps, what):
    """-> the list of what is wrong with stats12 ``st`` for this problem (empty: nothing).
    - v against the oracle: the solve's float64 v within 1e-9 max|v| before its one rounding to fp32, i.e. |v32 - v64| <= 2^-23 |v64| +
      1e-9 max|v64|;
    - support size and flag equal the oracle's; the slots behind K and [10], [11] are zero;
    - the KKT conditions from the returned v, in float64 (u = v - margin, w = P u + q', s_k = sum_j |P_kj| |u_j| + |q'_k|): u_k >= 0
      exactly, -w_k <= tol_k off the support and |u_k w_k| <= max|u| tol_k, with tol_k = 1e-8 s_k + 2^-24 sum_j |P_kj| |v_j|.  The second
      term is what the rounding of v to fp32 can move w_k by: stats12 is fp32, so a residual computed from it cannot be below that,
      however exact the solve was before the rounding.  (Measured on an MI355X over the SPD suite: the plain residual, without the
      second term, is 4.3e-8 relative at worst -- above 1e-8 and below the fp32 unit roundoff 6e-8, as the rounding predicts.)"""
    K = gram.shape[0] - 1
    s = G.gem_solve(gram, margin, eps)
    bad = []
    v = st[:K].astype(np.float64)
    if not (st[K:8] == 0).all() or st[10] != 0 or st[11] != 0:
        bad.append(f"{what}: slots behind K / [10..11] not zero: {st}")
    if st[8] != float(s["violated"]) or st[9] != float(s["support"]):
        bad.append(f"{what}: flag / support {st[8]} / {st[9]}, oracle {s['violated']} / {s['support']} (mask {s['mask']:b})")
    tol = 2.0 ** -23 * np.abs(s["v"]) + 1e-9 * np.abs(s["v"]).max()
    if not (np.abs(v - s["v"]) <= tol).all():
        bad.append(f"{what}: v {v} against {s['v']}: worst excess {float((np.abs(v - s['v']) - tol).max()):.3e}")
    if s["violated"]:
        P, qp = s["P"], s["qp"]
        u = v - margin
        w = P @ u + qp
        sk = np.abs(P) @ np.abs(u) + np.abs(qp)
        tk = 1e-8 * sk + U24 * (np.abs(P) @ np.abs(v))
        umax = np.abs(u).max() or 1.0
        off = u == 0
        literal = max(float((np.maximum(-w, 0) / sk)[off].max()) if off.any() else 0.0, float((np.abs(u * w) / (umax * sk)).max()))
        _check_against_oracle.worst = max(getattr(_check_against_oracle, "worst", 0.0), literal)
        if not (u >= 0).all():
            bad.append(f"{what}: v below the margin: {v}")
        if not ((-w <= tk) | ~off).all() or not (np.abs(u * w) <= umax * tk).all():
            bad.append(f"{what}: KKT residual {literal:.3e} relative (w {w}, u {u})")
    return bad


def test_gem_solve_not_violated_gives_zeros():
    rng = np.random.default_rng(5)
    for K in (1, 3, 8):
        A = rng.standard_normal((K, K + 2))
        st = _solve(_gram_of(A @ A.T, np.abs(rng.standard_normal(K)) * (rng.random(K) > 0.3)), 0.5, 1e-3)   # some q_k exactly 0
        assert (st == 0).all(), st


@pytest.mark.parametrize("margin,eps", [(0.0, 0.0), (0.5, 1e-3), (0.0, 1e-3), (0.5, 0.0)])
def test_gem_solve_closed_forms(margin, eps):
    """K = 1: v = max(margin, -q / (P + eps)); a diagonal P: the same per constraint (K = 8, mixed signs of q)."""
    bad = []
    for p, q in ((4.0, -3.0), (85.0, -1.6), (0.25, -7.0), (1e-3, -1e-4)):
        gram = _gram_of(np.array([[p]]), np.array([q]))
        st = _solve(gram, margin, eps)
        want = max(margin, -q / (p + eps))
        if abs(st[0] - want) > 2.0 ** -23 * want or st[8] != 1.0 or st[9] != float(-q / (p + eps) > margin):
            bad.append(("K = 1", p, q, st, want))
        bad += _check_against_oracle(st, gram, margin, eps, f"K = 1 p {p} q {q}")
    d = np.array([1.0, 4.0, 0.25, 9.0, 2.0, 0.5, 3.0, 7.0])
    q = np.array([-3.0, 2.0, -0.05, -1.0, -8.0, 0.9, 1.5, -0.7])
    gram = _gram_of(np.diag(d), q)
    st = _solve(gram, margin, eps)
    want = np.maximum(margin, -q / (d + eps))
    if not (np.abs(st[:8] - want) <= 2.0 ** -23 * np.abs(want)).all() or st[8] != 1.0 or st[9] != float((-q / (d + eps) > margin).sum()):
        bad.append(("diagonal", st, want))
    bad += _check_against_oracle(st, gram, margin, eps, "diagonal")
    assert not bad, bad


def test_gem_solve_random_spd_suite():
    """K = 2 .. 8 x 11 problems at condition number 1e6, supports of every size (K = 8 with all eight included), margin 0 and 0.5
    (tests/gem_ref.py::solve_suite; its decisions are checked to be clear of the tolerances by tests/test_gem_ref.py).  Asserted over
    the suite: every case runs, the failures are listed together."""
    _check_against_oracle.worst = 0.0
    bad, sizes = [], set()
    for K, seed, margin, gram, active in G.solve_suite():
        st = _solve(gram, margin, 0.0)
        again = _solve(gram, margin, 0.0)
        if st.tobytes() != again.tobytes():
            bad.append(f"K {K} seed {seed}: not the same bits run to run")
        bad += _check_against_oracle(st, gram, margin, 0.0, f"K {K} seed {seed} margin {margin}")
        sizes.add((K, int(st[9])))
    print(f"[gem] solve suite: worst KKT residual from the fp32 v, relative: {_check_against_oracle.worst:.3e}")
    assert not bad, "\n".join(bad)
    assert sizes >= {(K, n) for K in range(2, 9) for n in range(K + 1)}


@pytest.mark.parametrize("margin", [0.0, 0.5])
def test_gem_solve_duplicate_references_without_eps(margin):
    """r_1 = r_2 (equal Gram rows to the bit) and eps = 0: the singular support is skipped, the tie goes to the lower mask."""
    rng = np.random.default_rng(21)
    g, r, r3 = rng.standard_normal((3, 4097))
    r = -np.sign(np.dot(g, r)) * r
    refs = [r, r.copy(), r3]
    gram, _ = G.gem_gram(g, refs)
    assert gram[1, 1] == gram[1, 2] == gram[2, 2] and gram[0, 1] == gram[0, 2]
    st = _solve(gram, margin, 0.0)
    assert not _check_against_oracle(st, gram, margin, 0.0, "duplicates")
    lim = G.gem_solve(gram, margin, 1e-9 * gram[1, 1])
    a, b = (sum(v * x for v, x in zip(vv, refs)) for vv in (st[:3].astype(np.float64), lim["v"]))
    assert np.abs(a - b).max() <= 2.0 ** -22 * np.abs(b).max()   # fp32 coefficients against the limit's float64 ones


def test_gem_solve_does_not_hide_a_non_finite_entry():
    gram, _ = G.spd_problem(3, 0)
    for i, j, bad in ((1, 2, np.nan), (0, 2, np.inf), (0, 0, np.nan)):
        m = gram.copy()
        m[i, j] = m[j, i] = bad
        st = _solve(m, 0.5, 1e-3)
        assert np.isnan(st[:3]).all() and (st[3:8] == 0).all() and st[8] == 1.0 and (st[9:] == 0).all(), st


# ---- project ----------------------------------------------------------------------------------------------------------------------
def _stats(K, violated, seed=0):
    gen = torch.Generator().manual_seed(50 + seed)
    st = torch.zeros(12)
    st[:K] = 2 * torch.rand(K, generator=gen) - 1
    st[8] = float(violated)
    st[9] = float(K)
    return st.to(DEV)


@pytest.mark.parametrize("n,K", GRID)
def test_gem_project_vs_fp64(n, K):
    from mafed_amd import ops
    g, refs, g64, refs64 = _inputs(n, K)
    st = _stats(K, True, seed=K)
    nb = ops.gem_blocks(n)
    partials = torch.full((nb + 3,), -7.0, device=DEV)
    out = ops.gem_project(g, refs, st, sumsq_partials=partials)
    # aliasing: into g's own buffer and into the last ref's, as the plugin does
    g2 = g.clone()
    out_g = ops.gem_project(g2, refs, st, out=g2)
    refs2 = refs[:-1] + [refs[-1].clone()]
    p2 = torch.full((nb + 3,), -7.0, device=DEV)
    out_r = ops.gem_project(g, refs2, st, out=refs2[-1], sumsq_partials=p2)
    torch.cuda.synchronize()
    assert n == 0 or (out_g.data_ptr() == g2.data_ptr() and out_r.data_ptr() == refs2[-1].data_ptr())
    assert torch.equal(_bits(out), _bits(out_g)) and torch.equal(_bits(out), _bits(out_r)) and torch.equal(_bits(partials), _bits(p2))
    v = st[:K].double().cpu().numpy()
    want = G.gem_project(g64, refs64, v, True) if n else g64
    mag = np.abs(g64) + sum(abs(vk) * np.abs(r) for vk, r in zip(v, refs64))
    err = np.abs(out.double().cpu().numpy() - want)
    bound = K * 2.0 ** -23 * mag
    assert bool((err <= bound).all()), f"out: worst excess {float((err - bound).max()):.3e}"
    # norm hand-over: the partials folded by gradnorm_finish against the one-pass norm of out
    assert 1 <= nb <= 2048 and bool((partials[nb:] == -7.0).all())
    folded = ops.gradnorm_finish(partials[:nb], 2.0, torch.empty(2, device=DEV))
    if n:
        one_pass = ops.gradnorm_clip(out, 2.0)
        for i, what in enumerate(("norm", "clip scale")):
            a, b = float(folded[i]), float(one_pass[i])
            assert abs(a - b) <= 1e-6 * abs(b), f"{what}: folded {a} vs one pass {b}"
    else:
        assert float(folded[0]) == 0.0 and float(folded[1]) == 1.0


@pytest.mark.parametrize("n,K", GRID)
def test_gem_project_not_violated_copies_g_and_reads_no_ref(n, K):
    from mafed_amd import ops
    g, refs, _, _ = _inputs(n, K)
    st = _stats(K, False)                                     # coefficients present, flag 0: the flag decides
    infs = [torch.full_like(g, float("inf")) for _ in range(K)]
    partials = torch.full((ops.gem_blocks(n) + 3,), -7.0, device=DEV)
    out = ops.gem_project(g, infs, st, sumsq_partials=partials)
    alias = infs[-1]
    ops.gem_project(g, infs, st, out=alias)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(g)) and torch.equal(_bits(alias), _bits(g))   # bit for bit: the -0.0 in g[2] stays -0.0
    if n > 2:
        assert int(_bits(out)[2]) == -2 ** 31
    if n:
        a, b = float(ops.gradnorm_finish(partials[:ops.gem_blocks(n)], 2.0, torch.empty(2, device=DEV))[0]), float(ops.gradnorm_clip(g, 2.0)[0])
        assert abs(a - b) <= 1e-6 * b


@pytest.mark.parametrize("n", [n for n in SIZES if n] + [BIG])
def test_gem_project_with_one_ref_is_agems(n):
    """K = 1 with A-GEM's alpha fed as -v: both are one fma per element, within the elementwise bound of each other."""
    from mafed_amd import ops
    g, refs, g64, refs64 = _inputs(n, 1)
    st = _stats(1, True, seed=3)
    st4 = torch.tensor([0.0, 1.0, -float(st[0]), 1.0], device=DEV)
    a = ops.gem_project(g, refs, st)
    b = ops.agem_project(g, refs[0], st4)
    torch.cuda.synchronize()
    bound = 2.0 ** -23 * (np.abs(g64) + abs(float(st[0])) * np.abs(refs64[0]))
    assert bool((np.abs(a.double().cpu().numpy() - b.double().cpu().numpy()) <= bound).all())


def test_gem_poisoned_coefficients_reach_the_norm():
    """NaN coefficients with the flag set (what the solve leaves for a non-finite Gram): out is non-finite and the folded norm marks the
    step as skipped."""
    from mafed_amd import ops
    g, refs, _, _ = _inputs(4 * 1024 + 1, 2)
    st = torch.zeros(12, device=DEV)
    st[:2] = float("nan")
    st[8] = 1.0
    partials = torch.zeros(ops.gem_blocks(g.numel()), device=DEV)
    out = ops.gem_project(g, refs, st, sumsq_partials=partials)
    folded = ops.gradnorm_finish(partials, 2.0, torch.empty(2, device=DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and not np.isfinite(float(folded[0])) and float(folded[1]) == -1.0


def test_gem_kernels_refuse_bad_arguments():
    from mafed_amd import _lib, ops
    g, refs, _, _ = _inputs(1023, 8)
    st = _stats(8, True)
    gram = torch.zeros(100, dtype=torch.float64, device=DEV)
    for bad in ([], refs + [refs[0]]):   # K = 0, K = 9
        with pytest.raises(_lib.MafedHipError):
            ops.gem_gram(g, bad)
        with pytest.raises(_lib.MafedHipError):
            ops.gem_project(g, bad, st)
        with pytest.raises(_lib.MafedHipError):
            ops.gem_solve(gram, len(bad), 0.5, 1e-3)
    with pytest.raises(_lib.MafedHipError):   # misaligned
        ops.gem_gram(g[1:], [r[1:] for r in refs[:2]])
    with pytest.raises(_lib.MafedHipError):
        ops.gem_gram(g[4:], [refs[0][4:], refs[1][1:-3]])
    with pytest.raises(_lib.MafedHipError):
        ops.gem_project(g[1:], [r[1:] for r in refs[:2]], st)
    lib = _lib.load()
    need = lib.mafed_gem_workspace_bytes(g.numel(), 8)
    assert need == 45 * 2048 * 4 and lib.mafed_gem_workspace_bytes(g.numel(), 1) == 3 * 2048 * 4
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    arr, K = ops._gem_refs(g, refs)
    with pytest.raises(_lib.MafedHipError):   # a short workspace
        _lib.check(lib.mafed_gem_gram(g.data_ptr(), arr, K, g.numel(), gram.data_ptr(), ws.data_ptr(), need - 4, ops._stream()), "mafed_gem_gram")
    _lib.check(lib.mafed_gem_gram(g.data_ptr(), arr, K, g.numel(), gram.data_ptr(), ws.data_ptr(), need, ops._stream()), "mafed_gem_gram")
    torch.cuda.synchronize()
