"""fp64 numpy oracle of the replay-memory selection kernels (mafed_select_greedy, include/mafed_hip.h).

``greedy`` restates the kernel's rules: the target vector v is rounded to fp32 before every scan (herding keeps it in fp64 between
picks, r := (r + mean) - X[p]; k-center copies the picked row), distances are direct differences summed in fp64, a row is eligible
while it is not picked and its score is not NaN, and the lowest index wins ties.  ``literal`` is the textbook definition of the two
selections with explicit means and minima and no incremental state.
"""
import numpy as np

HERDING, KCENTER = 0, 1


def fixture(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def sqdist(X, v):
    """sum_j (X[i, j] - fp32(v[j]))^2 in fp64"""
    v32 = np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = X.astype(np.float64) - v32[None, :]
        return (e * e).sum(axis=1)


def arg_best(scores, taken, minimise):
    """(row, relative margin to the runner-up) of the lexicographic best (score, row) among the eligible rows; (-1, inf) if none.
    margin = |best - runner-up| / max(|best|, |runner-up|) (0 for two zeros, inf when no second row is eligible)."""
    ok = ~taken & ~np.isnan(scores)
    if not ok.any():
        return -1, np.inf
    key = np.where(ok, scores if minimise else -scores, np.inf)
    p = int(np.argmin(key))                      # first occurrence: the lowest row among equals
    rest = key.copy()
    rest[p] = np.inf
    ok2 = ok.copy()
    ok2[p] = False
    if not ok2.any():
        return p, np.inf
    a, b = abs(float(key[p])), abs(float(rest[int(np.argmin(rest))]))
    if not (np.isfinite(a) and np.isfinite(b)):
        return p, (0.0 if a == b else np.inf)
    den = max(a, b)
    return p, (abs(a - b) / den if den > 0 else 0.0)


def greedy(X, mean, k, mode, prefix=None):
    """-> picks int64 [k], values fp64 [k], last_scores fp64 [n], margins fp64 [k].  ``prefix`` (optional): picks to take instead of
    the oracle's own (the kernel's), so that scores can be compared pick by pick along the kernel's path; -1 entries end it."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    X64 = X.astype(np.float64)
    mean = np.asarray(mean, dtype=np.float64)
    picks = np.full(k, -1, dtype=np.int64)
    values = np.full(k, np.nan)
    margins = np.full(k, np.inf)
    taken = np.zeros(n, dtype=bool)
    r = mean.copy()
    m = np.full(n, np.inf)
    scores = np.full(n, np.nan)
    v = mean
    for t in range(k):
        dist = sqdist(X, v)
        if mode == HERDING or t == 0:
            scores, minimise = dist, True
        else:
            with np.errstate(invalid="ignore"):
                m = np.where(np.isnan(dist) | np.isnan(m), np.nan, np.minimum(m, dist))
            scores, minimise = m, False
        p, margins[t] = arg_best(scores, taken, minimise)
        if prefix is not None:
            p = int(prefix[t])
        if p < 0:
            break
        picks[t], values[t] = p, scores[p]
        taken[p] = True
        if mode == HERDING:
            r = (r + mean) - X64[p]
            v = r
        else:
            v = X64[p]
    return picks, values, scores, margins


def literal(X, k, mode):
    """The textbook selections in fp64 -> picks [k].  herding (iCaRL): argmin_i || mu - (x_i + sum of the chosen) / (t + 1) ||;
    k-center greedy: the row nearest mu, then argmax_i min_c || x_i - x_c || over the chosen centres c.  Lowest index on ties."""
    X64 = np.asarray(X, dtype=np.float64)
    n = X64.shape[0]
    mu = X64.mean(axis=0)
    chosen = []
    for t in range(k):
        free = [i for i in range(n) if i not in chosen]
        if mode == HERDING:
            total = X64[chosen].sum(axis=0) if chosen else 0.0
            cost = [float(np.sum((mu - (X64[i] + total) / (t + 1)) ** 2)) for i in free]
            chosen.append(free[int(np.argmin(cost))])
        elif t == 0:
            chosen.append(free[int(np.argmin([float(np.sum((X64[i] - mu) ** 2)) for i in free]))])
        else:
            cover = [min(float(np.sum((X64[i] - X64[c]) ** 2)) for c in chosen) for i in free]
            chosen.append(free[int(np.argmax(cover))])
    return np.asarray(chosen, dtype=np.int64)


# exact-pick fixtures: (mode, seed, n, d, k); the relative margin of every pick is >= 1e-3 (tests/test_select_ref.py), four times the
# worst-case fp32 error (d + 3) 2^-23 of a score at d = 2048, so the kernel's fp32 scores must order the rows as the oracle's do
EXACT_FIXTURES = ([(HERDING, s, 64, 4, 64) for s in (0, 2, 3, 4)] + [(KCENTER, s, 64, 4, 64) for s in (0, 2)] +
                  [(HERDING, s, 257, 130, 40) for s in (2, 3)])
