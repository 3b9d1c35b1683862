"""The task-vector merge passes (csrc/merge.hip: mafed_merge_fold / _ties_hist / _ties_fold / _apply) through the ops wrappers against the
numpy restatement (tests/merge_ref.py): every pass bit for bit, twice, and the two runs with the same bits.

The inputs keep every difference and sum out of the denormal range (asserted below), so the comparison does not depend on the denormal
mode of either machine."""
import numpy as np
import pytest
import torch

from tests.merge_ref import F, apply_ref, drop_of, fold_ref, same_bits, task_vector, ties_delta_ref, ties_fold_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

# 0: empty; 1, 3: scalar tail only; 4: one vector; 15: vectors and a tail; 16, 17: around a group of four vectors; 1023: less than one block;
# 4097: several blocks and a tail; 3 * 2^21 + 5: above 2 * 2048 * 256 vectors, so the grid-stride loop at the grid cap goes through its
# two-vector body, its one-vector body and the tail
SIZES = [0, 1, 3, 4, 15, 16, 17, 1023, 4097, 3 * 2 ** 21 + 5]
_INPUTS = {}


def _dev(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).to(DEV)
    return torch.from_numpy(a.copy()).to(DEV)


def _host(t):
    """Device tensor -> numpy with the same bits (bf16 as uint16 patterns)."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _exact_bits(a, b):
    """Run to run: the very same bits, NaN payloads included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    w = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
    return a.shape == b.shape and np.array_equal(a.view(w[a.itemsize]), b.view(w[b.itemsize]))


def _no_denormals(*arrays):
    for a in arrays:
        mag = np.abs(a[np.isfinite(a)])
        assert not ((mag > 0) & (mag < np.finfo(F).tiny)).any()


def _specials(buf, shift):
    for j, special in enumerate((-0.0, np.inf, np.nan, -np.inf)):
        buf[(7 * j + shift)::29] = special


def _inputs(n):
    """numpy {base, theta1, theta2, acc, shadow} for n elements, built once and left unchanged.  base is finite; theta1 carries -0.0, +-inf
    and NaN, acc the same at other places; every 11th element has theta1 == base; every 13th is a magmax tie: tau2 == -tau1 exactly
    (dyadic values) over an acc of zero."""
    if n not in _INPUTS:
        rng = np.random.default_rng(2000 + n % 997)
        base, theta1, theta2, acc = (rng.standard_normal(n).astype(F) for _ in range(4))
        _specials(theta1, 0)
        _specials(acc, 3)
        theta2[2::31] = np.inf
        theta1[4::11] = base[4::11]
        i = np.arange(n)[5::13]
        step = ((1 + i % 5) / 8.0).astype(F)
        base[5::13] = ((i % 7) / 4.0).astype(F)
        theta1[5::13] = base[5::13] + step
        theta2[5::13] = base[5::13] - step
        acc[5::13] = 0.0
        _no_denormals(task_vector(theta1, base), task_vector(theta2, base))
        _INPUTS[n] = dict(base=base, theta1=theta1, theta2=theta2, acc=acc, shadow=rng.integers(0, 2 ** 16, size=n).astype(np.uint16))
    return _INPUTS[n]


# ---- sum and magmax -------------------------------------------------------------------------------------------------------------------
def _fold_twice(x, rule):
    from mafed_amd import ops
    theta1, theta2, base, acc = _dev(x["theta1"]), _dev(x["theta2"]), _dev(x["base"]), _dev(x["acc"])
    ops.merge_fold_(theta1, base, acc, rule)
    first = _host(acc)
    ops.merge_fold_(theta2, base, acc, rule)
    assert _exact_bits(_host(theta1), x["theta1"]) and _exact_bits(_host(base), x["base"])      # the inputs are only read
    return first, _host(acc)


@pytest.mark.parametrize("rule", ["sum", "magmax"])
@pytest.mark.parametrize("n", SIZES)
def test_merge_fold(n, rule):
    x = _inputs(n)
    want1 = fold_ref(rule, x["theta1"], x["base"], x["acc"])
    want2 = fold_ref(rule, x["theta2"], x["base"], want1)
    _no_denormals(want1, want2)
    got, again = _fold_twice(x, rule), _fold_twice(x, rule)
    for a, b, w, what in zip(got, again, (want1, want2), ("first fold", "second fold")):
        assert _exact_bits(a, b), f"{what}: two runs differ"
        assert same_bits(a, w), f"{what} differs from the restatement"
    if rule == "magmax" and n > 13:
        tie = np.zeros(n, bool)
        tie[5::13] = True
        tau1, tau2 = task_vector(x["theta1"], x["base"]), task_vector(x["theta2"], x["base"])
        assert (tau2[tie] == -tau1[tie]).all() and (tau1[tie] != 0).all()
        assert _exact_bits(got[1][tie], tau1[tie])                                               # a tie keeps the earlier task
        nan_acc = np.isnan(x["acc"])
        assert np.isnan(got[1][nan_acc]).all()                                                   # a NaN acc never leaves
        nan_tau = np.isnan(tau1) & ~nan_acc
        assert _exact_bits(got[0][nan_tau], x["acc"][nan_tau])                                   # a NaN tau never wins


# ---- TIES -----------------------------------------------------------------------------------------------------------------------------
# One table: length 1, length 5, odd offsets and ends throughout, gaps of 3 or 4 elements that belong to no segment (the padding), 4096
# elements with a quarter of the magnitudes on one value, 70 001 elements (several blocks), 2^21 + 7 elements, a short one at the end.
QUARTER = 2


def _segment_table():
    lengths = [1, 5, 4096, 70001, 2 ** 21 + 7, 37]
    segs, off = [], 5
    for length in lengths:
        segs.append((off, length))
        off += length + 3 + (off + length) % 2          # the next offset is odd
    return segs, segs[-1][0] + segs[-1][1] + 6          # (and six elements of padding behind the last)


SEGMENTS, N_TIES = _segment_table()
DENSITIES = [1.0, 0.5, 0.2, 1e-7]                       # 1e-7: r = floor((1 - 1e-7) m) = m - 1 for every 1 < m < 10^7
_TIES = {}


def _ties_inputs():
    """numpy {base, thetas[3], covered}: three tasks with mixed signs (so that both counters reach 2), theta == base on every 11th element,
    -0.0, +-inf and NaN in theta of task 0.  In segment QUARTER the magnitudes of every task are 1536 values below 1, 1024 times 1.0 and
    1536 values above 1: at density 0.5 the threshold (rank 2048) is 1.0 and all 1024 go."""
    if not _TIES:
        rng = np.random.default_rng(77)
        base = rng.standard_normal(N_TIES).astype(F)
        thetas = [(base + (0.05 * rng.standard_normal(N_TIES)).astype(F)).astype(F) for _ in range(3)]
        for th in thetas:
            th[4::11] = base[4::11]
        _specials(thetas[0], 1)
        off, length = SEGMENTS[QUARTER]                 # (built last: no special and no zero difference in this segment)
        assert length == 4096
        base[off:off + length] = np.round(base[off:off + length] * 4) / 4              # multiples of 1/4: base +- 1.0 is exact
        for t in range(3):
            mag = np.concatenate([rng.uniform(0.1, 0.9, 1536), np.ones(1024), rng.uniform(1.1, 1.9, 1536)])
            tau = (rng.permutation(mag) * rng.choice([-1.0, 1.0], length)).astype(F)
            thetas[t][off:off + length] = base[off:off + length] + tau
            got = np.abs(task_vector(thetas[t], base)[off:off + length])
            assert int((got == 1.0).sum()) == 1024 and int((got < 1.0).sum()) == 1536
        covered = np.zeros(N_TIES, bool)
        for o, m in SEGMENTS:
            covered[o:o + m] = True
        assert 0 < int((~covered).sum()) < 40
        _no_denormals(*[task_vector(th, base) for th in thetas])
        _TIES.update(base=base, thetas=thetas, covered=covered)
    return _TIES


def _ties_start(covered):
    """pos, neg, counts in front of the first fold: zero inside the segments, sentinels on the padding (which no fold may touch)."""
    pos, neg = np.where(covered, 0.0, 7.0).astype(F), np.where(covered, 0.0, -3.0).astype(F)
    counts = np.where(covered[:, None], 0, 9).astype(np.uint8) * np.ones((1, 2), np.uint8)
    return pos, neg, np.ascontiguousarray(counts)


def _ties_run(x, density, blocks):
    from mafed_amd import ops
    base, thetas = _dev(x["base"]), [_dev(th) for th in x["thetas"]]
    pos, neg, counts = (_dev(a) for a in _ties_start(x["covered"]))
    seg = torch.tensor(SEGMENTS, dtype=torch.int64, device=DEV)
    out = []
    for th in thetas:
        stats = ops.merge_ties_fold_(th, base, pos, neg, counts, seg, blocks, drop_of(density))
        out.append((_host(pos), _host(neg), _host(counts), _host(stats)))
    assert _exact_bits(_host(base), x["base"]) and all(_exact_bits(_host(a), b) for a, b in zip(thetas, x["thetas"]))
    return out


@pytest.mark.parametrize("density", DENSITIES, ids=["d1", "d05", "d02", "dmin"])
def test_merge_ties_fold(density):
    from mafed_amd import ops
    x = _ties_inputs()
    pos, neg, counts = _ties_start(x["covered"])
    want = []
    for th in x["thetas"]:
        pos, neg, counts, stats = ties_fold_ref(th, x["base"], pos, neg, counts, SEGMENTS, drop_of(density))
        want.append((pos, neg, counts, stats))
    _no_denormals(pos, neg)
    default = ops.merge_select_blocks(max(m for _, m in SEGMENTS))
    assert default == 512 and 70001 // 4 > 4 * 3 * 256   # 70 001 elements: several blocks in one trip by default, several trips at 3 blocks
    runs = [_ties_run(x, density, default), _ties_run(x, density, default)]
    if density == 0.5:
        runs.append(_ties_run(x, density, 3))           # another grid: the same bits again
    for fold in range(3):
        for name, k in (("pos", 0), ("neg", 1), ("counts", 2), ("stats", 3)):
            for run in runs[1:]:
                assert _exact_bits(runs[0][fold][k], run[fold][k]), f"fold {fold}, {name}: two runs differ"
            assert same_bits(runs[0][fold][k], want[fold][k]), f"fold {fold}, {name} differs from the restatement"
    pos, neg, counts, stats = runs[0][2]
    print(f"[merge] ties density {density}: m {stats[:, 0].tolist()} r {stats[:, 1].tolist()} kept {stats[:, 2].tolist()}")
    if density >= 0.2:                                  # (at the smallest density a fold keeps at most one element of a segment)
        assert int(counts[x["covered"], 0].max()) >= 2 and int(counts[x["covered"], 1].max()) >= 2    # both counters reach 2 somewhere
    pad = ~x["covered"]
    assert (pos[pad] == 7.0).all() and (neg[pad] == -3.0).all() and (counts[pad] == 9).all()   # the padding is not touched
    for (off, m), row in zip(SEGMENTS, stats):
        assert row[0] == m and row[1] == min(int(np.floor(np.float64(drop_of(density)) * np.float64(m))), m)
    assert stats[0].tolist()[:3] == [1, 0, 1]           # length 1: r = 0, kept whatever the density
    if density == 1e-7:
        assert all(row[1] == m - 1 for (_, m), row in zip(SEGMENTS[1:], stats[1:]))
    if density == 0.5:
        row = stats[QUARTER]
        assert row[1] == 2048 and row[3] == 0x3F800000 and row[2] == 1536, row.tolist()   # the 1024 ties at the threshold all go


# ---- apply ----------------------------------------------------------------------------------------------------------------------------
def _apply_state(n, rule):
    """numpy (acc or pos, neg, counts): a state as folds leave it -- for ties, pos > 0 with npos >= 1 or +0.0 with npos == 0 (neg alike),
    a third of the elements with both counters zero; for sum / magmax the acc of ``_inputs`` with its -0.0, +-inf and NaN."""
    x = _inputs(n)
    if rule != "ties":
        return x["acc"], None, None
    rng = np.random.default_rng(3000 + n % 997)
    counts = rng.integers(0, 4, size=(n, 2)).astype(np.uint8)
    counts[rng.integers(0, 3, size=n) == 0] = 0
    pos = np.where(counts[:, 0] > 0, np.abs(rng.standard_normal(n)) + 0.01, 0.0).astype(F)
    neg = np.where(counts[:, 1] > 0, -np.abs(rng.standard_normal(n)) - 0.01, 0.0).astype(F)
    both = (counts[:, 0] > 0) & (counts[:, 1] > 0)
    neg[both & (np.arange(n) % 5 == 0)] = -pos[both & (np.arange(n) % 5 == 0)]      # a dead heat: d = +0.0
    pos[(counts[:, 0] > 0) & (np.arange(n) % 17 == 2)] = np.inf
    return pos, neg, counts


@pytest.mark.parametrize("rule", ["sum", "magmax", "ties"])
@pytest.mark.parametrize("n", SIZES)
def test_merge_apply(n, rule):
    from mafed_amd import ops
    x = _inputs(n)
    acc, neg, counts = _apply_state(n, rule)
    d = ties_delta_ref(acc, neg, counts) if rule == "ties" else acc
    base_d, acc_d = _dev(x["base"]), _dev(acc)
    extra = dict(neg=_dev(neg), counts=_dev(counts)) if rule == "ties" else {}
    for scaling in (1.0, 0.3, 0.0):
        for with_shadow in (True, False):
            want_p, want_sh = apply_ref(x["base"], d, scaling, shadow=with_shadow)
            with np.errstate(all="ignore"):             # (0 * inf)
                _no_denormals(want_p, (F(scaling) * d).astype(F))
            got = []
            for _ in range(2):
                p, sh = _dev(x["theta1"]), (_dev(x["shadow"]) if with_shadow else None)
                ops.merge_apply_(p, sh, base_d, acc_d, rule, scaling, **extra)
                got.append((_host(p), _host(sh) if with_shadow else None))
            what = f"scaling {scaling}, {'shadow' if with_shadow else 'no shadow'}"
            assert _exact_bits(got[0][0], got[1][0]), f"{what}: two runs differ"
            assert same_bits(got[0][0], want_p), f"{what}: p differs from the restatement"
            if with_shadow:
                assert _exact_bits(got[0][1], got[1][1]) and same_bits(got[0][1], want_sh), f"{what}: shadow"
                if n:                                   # the rounding is the one ops.cast gives
                    assert _exact_bits(got[0][1], _host(ops.cast(_dev(got[0][0]), torch.bfloat16)))
            if rule == "ties":
                dead = (counts[:, 0] == 0) & (counts[:, 1] == 0)
                assert _exact_bits(got[0][0][dead], x["base"][dead])            # no task voted: base
    assert _exact_bits(_host(base_d), x["base"]) and _exact_bits(_host(acc_d), acc)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_merge_passes_refuse_misaligned_and_mismatched_buffers():
    from mafed_amd import _lib, ops
    n = 1023
    x = _inputs(n)
    theta, base, acc, sh = (_dev(x[k]) for k in ("theta1", "base", "acc", "shadow"))
    pos, neg = _dev(x["acc"]), _dev(x["theta2"])
    counts = torch.full((n, 2), 5, dtype=torch.uint8, device=DEV)
    seg = torch.tensor([[0, 100]], dtype=torch.int64, device=DEV)
    flat_counts = counts.view(-1)
    calls = [
        lambda: ops.merge_fold_(theta[1:], base[1:], acc[1:], "sum"), lambda: ops.merge_fold_(theta[2:], base[2:], acc[2:], "magmax"),
        lambda: ops.merge_fold_(theta[4:], base, acc, "sum"), lambda: ops.merge_fold_(theta, base, acc[:-1], "magmax"),
        lambda: ops.merge_ties_fold_(theta[1:], base[1:], pos[1:], neg[1:], flat_counts[2:].view(-1, 2), seg, 1, 0.5),
        lambda: ops.merge_ties_fold_(theta, base, pos, neg[:-4], counts, seg, 1, 0.5),
        lambda: ops.merge_ties_fold_(theta, base, pos, neg, counts[:-1], seg, 1, 0.5),
        lambda: ops.merge_apply_(acc[1:], sh[1:], base[1:], theta[1:], "sum", 1.0),
        lambda: ops.merge_apply_(acc, sh[:-1], base, theta, "magmax", 1.0), lambda: ops.merge_apply_(acc, None, base[4:], theta, "sum", 1.0),
        lambda: ops.merge_apply_(acc[3:], None, base[3:], pos[3:], "ties", 1.0, neg=neg[3:], counts=flat_counts[6:].view(-1, 2)),
        lambda: ops.merge_apply_(acc, sh, base, pos, "ties", 1.0, neg=neg, counts=counts[:-2]),
        lambda: ops.merge_apply_(acc, sh, base, pos, "ties", 1.0), lambda: ops.merge_apply_(acc, sh, base, pos, "sum", 1.0, neg=neg, counts=counts),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(_lib.MafedHipError):
            call()
    torch.cuda.synchronize()
    for t, k in ((theta, "theta1"), (base, "base"), (acc, "acc"), (sh, "shadow"), (pos, "acc"), (neg, "theta2")):
        assert _exact_bits(_host(t), x[k])              # nothing was launched
    assert bool((counts == 5).all())
