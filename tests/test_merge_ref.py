"""CPU: the streaming numpy restatement of the task-vector merge (tests/merge_ref.py) against an independent *batch*
formulation built from the stacked [T, n] task vectors -- what the papers write down."""
import numpy as np
import pytest

from tests.merge_ref import F, MergeRef, apply_ref, drop_of, same_bits, task_vector
from tests.packnet_ref import mag_bits

T, N = 4, 4000   # T = 4: a sequential fp32 sum of at most 4 same-signed terms and one division stay within 2 ulp of the exact mean
SEGMENTS = [(0, 1), (1, 5), (6, 1500), (1509, N - 1509)]   # elements 1506 .. 1508 lie in no segment, as the flat buffer's padding does


def _case(seed=3):
    """base and T fine-tuned parameter vectors.  At every element the T magnitudes come from T bands 0.01 * 3^b * [1, 1.3], one band per
    task (which, differs from element to element): the largest of any subset exceeds the sum of the others by 0.35 of itself, so no kept
    mass sums to within 0.0035 of zero.  A task is drawn again until no two of its |tau| inside a segment are equal."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(N).astype(F)
    shift = rng.integers(0, T, N)
    thetas = []
    for t in range(T):
        while True:
            mag = 0.01 * 3.0 ** ((t + shift) % T) * rng.uniform(1.0, 1.3, N)
            theta = (base + (mag * rng.choice([-1.0, 1.0], N)).astype(F)).astype(F)
            bits = mag_bits(task_vector(theta, base))
            if all(np.unique(bits[off:off + length]).size == length for off, length in SEGMENTS):
                break
        thetas.append(theta)
    return base, thetas


def _run(rule, base, thetas, density=0.2):
    ref = MergeRef(rule, density=density, segments=SEGMENTS)
    ref.begin(base)
    for th in thetas:
        ref.update(th)
    return ref


def test_sum_is_the_sequential_fp32_sum():
    base, thetas = _case()
    ref = _run("sum", base, thetas)
    taus = np.stack([task_vector(th, base) for th in thetas])
    want = np.zeros(N, F)
    for t in range(T):
        want = (want + taus[t]).astype(F)
    assert same_bits(ref.acc, want) and ref.task_id == T
    assert np.abs(ref.acc.astype(np.float64) - taus.astype(np.float64).sum(0)).max() < 1e-5


def test_magmax_takes_the_largest_magnitude_and_the_first_on_a_tie():
    base, thetas = _case()
    thetas = [th.copy() for th in thetas]
    # ties: task 3 repeats task 1's |tau| with the other sign on every 7th element, and both are made the largest there.  The mirrored
    # value is base - tau, whose difference from base is -tau only where the subtraction is exact: keep those elements
    tau1 = task_vector(thetas[1], base) * F(4.0)
    thetas[1][::7] = (base + tau1)[::7]
    tau1 = task_vector(thetas[1], base)
    thetas[3][::7] = (base - tau1)[::7]
    taus = np.stack([task_vector(th, base) for th in thetas])
    tied = np.zeros(N, bool)
    tied[::7] = True
    tied &= (taus[3] == -taus[1]) & (np.abs(taus[1]) > np.abs(np.delete(taus, [1, 3], 0)).max(0))
    assert tied.sum() > 100
    ref = _run("magmax", base, thetas)
    first_max = np.argmax(np.abs(taus), axis=0)        # argmax returns the first of equal maxima
    want = taus[first_max, np.arange(N)]
    assert same_bits(ref.acc, want)
    assert (np.abs(ref.acc) == np.abs(taus).max(0)).all()
    assert (first_max[tied] == 1).all() and same_bits(ref.acc[tied], taus[1][tied])


def test_magmax_nan_rules():
    base = np.zeros(4, F)
    ref = MergeRef("magmax")
    ref.begin(base)
    ref.update(np.array([1.0, np.nan, -2.0, 0.5], F))
    assert same_bits(ref.acc, np.array([1.0, 0.0, -2.0, 0.5], F))      # a NaN tau never wins
    ref.acc[3] = np.nan
    ref.update(np.array([-3.0, 1.0, 2.0, 9.0], F))
    assert same_bits(ref.acc[:3], np.array([-3.0, 1.0, -2.0], F)) and np.isnan(ref.acc[3])   # a tie keeps the earlier; a NaN acc never leaves


def _batch_ties(base, thetas, density):
    """float64, from the stacked vectors: trim per segment by sorting, elect by the sign of the summed kept mass, mean over the tasks that
    agree.  -> (elected sign [n], contributing [T, n] bool, mean [n] float64, kept [T, n], r per segment)."""
    taus = np.stack([task_vector(th, base) for th in thetas]).astype(np.float64)
    kept = np.zeros(taus.shape, bool)
    rs = []
    for off, length in SEGMENTS:
        r = int(np.floor(drop_of(density) * length))
        rs.append(r)
        for t in range(len(thetas)):
            a = np.abs(taus[t, off:off + length])
            kept[t, off:off + length] = True if r == 0 else a > np.sort(a)[r - 1]
    trimmed = np.where(kept, taus, 0.0)
    mass = trimmed.sum(0)
    sign = np.sign(mass)
    contrib = kept & (np.sign(taus) == sign) & (sign != 0)
    cnt = contrib.sum(0)
    mean = np.where(cnt > 0, np.where(contrib, taus, 0.0).sum(0) / np.maximum(cnt, 1), 0.0)
    return sign, contrib, mean, kept, rs, mass


@pytest.mark.parametrize("density", [0.2, 0.5, 1.0])
def test_ties_against_the_batch_formulation(density):
    base, thetas = _case()
    ref = _run("ties", base, thetas, density)
    sign, contrib, mean, kept, rs, mass = _batch_ties(base, thetas, density)
    covered = np.zeros(N, bool)
    for off, length in SEGMENTS:
        covered[off:off + length] = True
    live = kept.any(0)
    assert np.abs(mass[live]).min() > 1e-3, "the fixture must keep |pos + neg| away from zero, or fp32 and fp64 may elect differently"
    d = ref.delta()
    assert (np.sign(d.astype(np.float64)) == sign).all()
    up, down = (contrib & (sign > 0)).sum(0), (contrib & (sign < 0)).sum(0)
    npos_all = (kept & (np.stack([task_vector(th, base) for th in thetas]) > 0)).sum(0)
    nneg_all = (kept & (np.stack([task_vector(th, base) for th in thetas]) < 0)).sum(0)
    assert (ref.counts[:, 0] == npos_all).all() and (ref.counts[:, 1] == nneg_all).all()     # the set of kept tasks, by sign
    assert (np.where(sign > 0, ref.counts[:, 0], np.where(sign < 0, ref.counts[:, 1], 0)) == up + down).all()   # the contributing tasks
    ulp = np.spacing(np.abs(mean).astype(F)).astype(np.float64)
    err = np.abs(d.astype(np.float64) - mean)
    print(f"[merge] ties density {density}: worst mean error {float((err / ulp).max()):.3f} ulp")
    assert (err <= 2.0 * ulp).all()
    assert not ref.counts[~covered].any() and not ref.pos[~covered].any() and not ref.neg[~covered].any()
    # the last fold's statistics: no two |tau| of a task are equal inside a segment, so exactly m - r are kept
    last = task_vector(thetas[-1], base)
    for (off, length), row, r in zip(SEGMENTS, ref.stats, rs):
        assert np.unique(mag_bits(last[off:off + length])).size == length
        assert row[0] == length and row[1] == r and row[2] == length - r
    assert ref.stats[0].tolist()[:3] == [1, 0, 1]      # m = 1: r = floor(drop) = 0, everything kept


def test_ties_density_one_with_agreeing_signs_is_the_plain_mean():
    rng = np.random.default_rng(9)
    base = rng.standard_normal(N).astype(F)
    sign = rng.choice([-1.0, 1.0], N)
    thetas = [(base + (rng.uniform(0.01, 2.0, N) * sign).astype(F)).astype(F) for _ in range(T)]
    ref = _run("ties", base, thetas, density=1.0)
    taus = np.stack([task_vector(th, base) for th in thetas])
    covered = np.zeros(N, bool)
    for off, length in SEGMENTS:
        covered[off:off + length] = True
    assert ((ref.counts.sum(1) == T) == covered).all()
    want = taus.astype(np.float64).mean(0)
    d = ref.delta()
    ulp = np.spacing(np.abs(want).astype(F)).astype(np.float64)
    assert (np.abs(d.astype(np.float64) - want)[covered] <= 2.0 * ulp[covered]).all()
    assert same_bits(d[~covered], np.zeros(int((~covered).sum()), F))


@pytest.mark.parametrize("rule", ["sum", "magmax", "ties"])
def test_apply(rule):
    base, thetas = _case()
    ref = _run(rule, base, thetas)
    p0, sh0 = ref.merged(0.0, shadow=True)
    assert same_bits(p0, base)                          # scaling 0: base bit for bit (the fixture has no -0.0, which +0.0 would turn)
    p, _ = ref.merged(0.3)
    step = (F(0.3) * ref.delta()).astype(F)
    assert same_bits(p, (base + step).astype(F))
    fused = (base.astype(np.float64) + np.float64(F(0.3)) * ref.delta().astype(np.float64)).astype(F)
    assert not same_bits(p, fused)                      # rounded twice: a fused multiply-add would differ somewhere on 4000 elements
    fresh = MergeRef(rule, segments=SEGMENTS)
    fresh.begin(base)
    assert same_bits(fresh.merged(1.0)[0], base)        # before the first update the merged model is base itself
    assert same_bits(apply_ref(base, np.zeros(N, F), 1.0)[0], base)
