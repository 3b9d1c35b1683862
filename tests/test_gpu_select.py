"""GPU: the replay-memory selection kernels (csrc/select.hip, ops.select_greedy) against the fp64 oracle of tests/select_ref.py.

Picks are compared with the oracle's only on the fixtures whose margins tests/test_select_ref.py asserts; everywhere else a pick is
checked exactly against the kernel's own scores (it must be their lexicographic arg-best) and the scores against the oracle run along
the kernel's picks, at rtol = (d + 3) 2^-23: twice the worst-case error of a d-term fp32 sum of squares of rounded differences.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.select_ref import EXACT_FIXTURES, HERDING, KCENTER, fixture, greedy, sqdist

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = [HERDING, KCENTER]

# (n, d, k).  The issue's table, then the sizes at which the launch takes another path: n above 2048 blocks x 16 rows (grid cap: a
# wave walks several rows), d above 8192 (v read through the caches instead of LDS) with and without 16-byte loads.
SHAPES = [(1, 1, 1), (7, 3, 7), (1000, 64, 100), (4099, 1024, 48), (4099, 2048, 8), (513, 1026, 16),
          (40000, 8, 5), (64, 8196, 3), (33, 8195, 3)]
LAYOUTS = ["dense", "ld+4", "ld+1"]


def _rtol(d):
    return (d + 3) * 2.0 ** -23


def _device(Xh, layout="dense"):
    """Xh on the device; strided layouts are views into a wider buffer whose extra columns hold NaN (a read behind column d shows)."""
    n, d = Xh.shape
    if layout == "dense":
        return torch.from_numpy(Xh).to(DEV)
    base = torch.full((n, d + (4 if layout == "ld+4" else 1)), float("nan"), device=DEV)
    X = base[:, :d]
    X.copy_(torch.from_numpy(Xh))
    return X


def _mean(X):
    from mafed_amd import ops
    return ops.cka_stats(X, row_norms=False)[0][0]


def _run(X, mean, mode, k):
    from mafed_amd import ops
    picks, values, scores = ops.select_greedy(X, mean, mode, k, want_scores=True)
    return picks.cpu().numpy(), values.cpu().numpy(), scores.cpu().numpy()


def _arg_best(scores, earlier, minimise):
    ok = ~np.isnan(scores)
    ok[earlier[earlier >= 0]] = False
    if not ok.any():
        return -1
    best = scores[ok].min() if minimise else scores[ok].max()
    return int(np.flatnonzero(ok & (scores == best))[0])


def _check_last_pick(picks, values, scores, mode, what):
    K = len(picks)
    want = _arg_best(scores, picks[:K - 1], mode == HERDING or K == 1)
    assert picks[K - 1] == want, f"{what}: pick {K - 1} is {picks[K - 1]}, the arg-best of the kernel's scores is {want}"
    if want >= 0:
        assert values[K - 1].view(np.int32) == scores[want].view(np.int32), what


def _check_scores(Xh, mean_h, picks, values, scores, mode, what):
    d = Xh.shape[1]
    _, ref_values, ref_scores, _ = greedy(Xh, mean_h, len(picks), mode, prefix=picks)
    for name, got, ref in (("last_scores", scores, ref_scores), ("values", values, ref_values)):
        err = np.abs(got.astype(np.float64) - ref)
        bound = _rtol(d) * np.abs(ref)
        worst = float((err / np.maximum(np.abs(ref), 1e-300)).max()) if err.size else 0.0
        print(f"[select] {what} {name}: worst rel err {worst:.3e} (bound {_rtol(d):.3e})")
        assert not np.isnan(got).any() and bool((err <= bound).all()), f"{what} {name}: rel err {worst:.3e} > {_rtol(d):.3e}"


@pytest.mark.parametrize("mode,seed,n,d,k", EXACT_FIXTURES)
def test_exact_picks(mode, seed, n, d, k):
    Xh = fixture(seed, n, d)
    X = _device(Xh)
    mean = _mean(X)
    picks, values, scores = _run(X, mean, mode, k)
    ref_picks, _, _, margins = greedy(Xh, mean.cpu().numpy(), k, mode)
    assert margins.min() >= 1e-3
    assert picks.tolist() == ref_picks.tolist()
    _check_scores(Xh, mean.cpu().numpy(), picks, values, scores, mode, f"exact {mode} seed {seed}")


@pytest.mark.parametrize("mode", MODES)
def test_every_pick_is_the_arg_best_of_the_kernels_scores(mode):
    n, d = 257, 130
    Xh = fixture(11, n, d)
    X = _device(Xh)
    mean = _mean(X)
    full, _, _ = _run(X, mean, mode, 12)
    for K in range(1, 13):
        picks, values, scores = _run(X, mean, mode, K)
        assert picks[:K - 1].tolist() == full[:K - 1].tolist()
        _check_last_pick(picks, values, scores, mode, f"mode {mode} K {K}")
    assert picks.tolist() == full.tolist()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_last_pick_and_scores(n, d, k, mode, layout):
    Xh = fixture(100 + n % 89 + d % 13, n, d)
    X = _device(Xh, layout)
    mean = _mean(X)
    picks, values, scores = _run(X, mean, mode, k)
    what = f"{n}x{d} k {k} mode {mode} {layout}"
    assert len(set(picks.tolist())) == k and picks.min() >= 0 and picks.max() < n, what
    _check_last_pick(picks, values, scores, mode, what)
    _check_scores(Xh, mean.cpu().numpy(), picks, values, scores, mode, what)


@pytest.mark.parametrize("mode", MODES)
def test_properties(mode):
    n, d = 1000, 64
    Xh = fixture(5, n, d)
    Xh[n - 2] = Xh[3]            # rows 3 and n - 2 are scanned by different blocks (63 blocks; row i goes to wave i mod 252)
    X = _device(Xh)
    mean = _mean(X)
    a = _run(X, mean, mode, n)
    b = _run(X, mean, mode, n)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
    picks, values, _ = a
    assert sorted(picks.tolist()) == list(range(n))           # k = n: a permutation
    order = picks.tolist()
    assert order.index(3) < order.index(n - 2)
    if mode == KCENTER:
        assert bool((np.diff(values[1:]) <= 0).all()) and values[-1] == 0.0    # (the duplicate is covered at radius 0)
    # k = 1: the row nearest the mean
    p1, v1, s1 = _run(X, mean, mode, 1)
    d64 = sqdist(Xh, mean.cpu().numpy())
    assert d64[p1[0]] <= d64.min() * (1 + 2 * _rtol(d)) and abs(v1[0] - d64[p1[0]]) <= _rtol(d) * d64[p1[0]]
    assert np.array_equal(s1.view(np.int32), _run(X, mean, HERDING, 1)[2].view(np.int32))   # k-center's first scan is herding's


@pytest.mark.parametrize("mode", MODES)
def test_nan_rows_are_never_picked(mode):
    n, d = 257, 12
    Xh = fixture(6, n, d)
    X = _device(Xh)
    mean = _mean(X)              # of the clean rows: a NaN row would make the mean, and with it every score, NaN
    bad = [0, 100, 256]
    X[bad, 5] = float("nan")
    picks, values, scores = _run(X, mean, mode, n)
    assert picks[-3:].tolist() == [-1, -1, -1] and bool(np.isnan(values[-3:]).all())
    assert sorted(picks[:-3].tolist()) == [i for i in range(n) if i not in bad]
    assert bool(np.isnan(scores[bad]).all()) and int(np.isnan(scores).sum()) == 3


def test_bad_arguments_return_error_codes():
    from mafed_amd import _lib, ops
    lib = _lib.load()
    n, d = 32, 8
    X = torch.randn(n, d, device=DEV)
    mean = _mean(X)
    picks = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    values = torch.full((n + 1,), -7.0, device=DEV)
    need = lib.mafed_select_workspace_bytes(n, d)
    assert need >= n * 8 + d * 12
    ws = ops.workspace(X.device).get(need)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(ops._stream())

    def call(k=4, ldx=d, mean_ptr=p(mean), ws_bytes=ws.numel(), mode=0):
        return lib.mafed_select_greedy(p(X), n, d, ldx, mean_ptr, mode, k, p(picks), p(values), None, p(ws), ws_bytes, st)

    assert call(k=n + 1) == -1 and call(k=0) == -1 and call(ldx=d - 1) == -1 and call(mean_ptr=None) == -1 and call(mode=2) == -1
    assert call(ws_bytes=need - 1) == -3
    assert lib.mafed_last_error_string()
    torch.cuda.synchronize()
    assert bool((picks == -7).all()) and bool((values == -7.0).all())      # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((picks[:4] >= 0).all()) and bool((picks[4:] == -7).all())
