"""A numpy restatement of the task-vector merge (mafed_amd/csrc/merge.hip): streaming, in fp32, one rounding per
operation exactly as the design states it -- np.float32 operations only.  The GPU tests compare bits.

IEEE 754 fixes every bit of a result except the sign and payload of a NaN: an x86 host makes 0xFFC00000 from inf - inf and from 0 * inf
where other machines make 0x7FC00000, so this restatement has no bits of its own there.  ``same_bits`` therefore asks for equal bits
wherever the expected value is a number, and for a NaN (any) wherever it is a NaN."""
import numpy as np

from tests.packnet_ref import bf16_bits, mag_bits, select_k

F = np.float32
RULES = ("sum", "magmax", "ties")


def same_bits(got, want):
    """Equal bit patterns; where ``want`` is a NaN, ``got`` must be a NaN.  fp32 arrays, bf16 patterns as uint16, or integer arrays."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.float32:
        g, w = got.view(np.uint32), want.view(np.uint32)
        gn, wn = (g & 0x7FFFFFFF) > 0x7F800000, (w & 0x7FFFFFFF) > 0x7F800000
    elif got.dtype == np.uint16:
        g, w = got, want
        gn, wn = (g & 0x7FFF) > 0x7F80, (w & 0x7FFF) > 0x7F80
    else:
        return np.array_equal(got, want)
    return bool(np.array_equal(gn, wn) and np.array_equal(g[~wn], w[~wn]))


def drop_of(density):
    """The trimmed share, computed once in Python double: the expression the plugin uses."""
    return 1.0 - density


def task_vector(theta, base):
    with np.errstate(all="ignore"):
        return (theta.astype(F) - base.astype(F)).astype(F)


def fold_ref(rule, theta, base, acc):
    """-> acc' of the rules sum and magmax."""
    tau = task_vector(theta, base)
    with np.errstate(all="ignore"):
        if rule == "sum":
            return (acc + tau).astype(F)
        return np.where(np.abs(tau) > np.abs(acc), tau, acc).astype(F)   # a NaN compares false: tau never wins, acc never leaves


def trim_ref(tau, segments, drop):
    """-> (kept [n] bool, stats int64 [S, 4] = {m, r, kept, tau_bits}).  Per segment (offset, length): the r = floor(drop * m) smallest
    patterns of |tau| go, and every element whose pattern equals the r-th smallest with them.  Outside every segment nothing is kept."""
    kept = np.zeros(tau.size, dtype=bool)
    stats = np.zeros((len(segments), 4), dtype=np.int64)
    for s, (off, length) in enumerate(segments):
        bits = mag_bits(tau[off:off + length])
        m = int(bits.size)
        r = min(select_k(m, drop), m)
        tau_bits = int(np.sort(bits, kind="stable")[r - 1]) if r > 0 else 0
        k = np.ones(m, dtype=bool) if r == 0 else bits > np.uint32(tau_bits)
        kept[off:off + length] = k
        stats[s] = m, r, int(k.sum()), tau_bits
    return kept, stats


def ties_fold_ref(theta, base, pos, neg, counts, segments, drop):
    """One TIES fold -> (pos', neg', counts' uint8 [n, 2] = {npos, nneg}, stats)."""
    tau = task_vector(theta, base)
    kept, stats = trim_ref(tau, segments, drop)
    with np.errstate(all="ignore"):
        up, down = kept & (tau > 0), kept & (tau < 0)
        pos2 = np.where(up, (pos + tau).astype(F), pos).astype(F)
        neg2 = np.where(down, (neg + tau).astype(F), neg).astype(F)
    counts2 = counts.copy()
    counts2[:, 0] += up.astype(np.uint8)
    counts2[:, 1] += down.astype(np.uint8)
    return pos2, neg2, counts2, stats


def ties_delta_ref(pos, neg, counts):
    """Elect and mean: the sign of the summed mass decides; a dead heat (or a NaN) gives +0.0."""
    with np.errstate(all="ignore"):
        s = (pos + neg).astype(F)
        mp = (pos / counts[:, 0].astype(F)).astype(F)
        mn = (neg / counts[:, 1].astype(F)).astype(F)
    return np.where(s > 0, mp, np.where(s < 0, mn, F(0.0))).astype(F)


def apply_ref(base, d, scaling, shadow=False):
    """-> (p, bf16 patterns of p or None): p = fl(base + fl(scaling * d)), rounded twice."""
    with np.errstate(all="ignore"):
        step = (F(scaling) * d.astype(F)).astype(F)
        p = (base.astype(F) + step).astype(F)
    return p, (bf16_bits(p) if shadow else None)


class MergeRef:
    """The plugin's state machine on numpy arrays: begin / update / merged."""

    def __init__(self, rule, density=0.2, segments=None):
        assert rule in RULES
        self.rule, self.density, self.segments, self.task_id = rule, density, segments, 0
        self.stats = None

    def begin(self, theta0):
        self.base = theta0.astype(F).copy()
        n = self.base.size
        if self.rule == "ties":
            self.pos, self.neg, self.counts = np.zeros(n, F), np.zeros(n, F), np.zeros((n, 2), np.uint8)
        else:
            self.acc = np.zeros(n, F)

    def update(self, theta):
        if self.rule == "ties":
            self.pos, self.neg, self.counts, self.stats = ties_fold_ref(theta, self.base, self.pos, self.neg, self.counts, self.segments,
                                                                        drop_of(self.density))
        else:
            self.acc = fold_ref(self.rule, theta, self.base, self.acc)
        self.task_id += 1

    def delta(self):
        return ties_delta_ref(self.pos, self.neg, self.counts) if self.rule == "ties" else self.acc

    def merged(self, scaling, shadow=False):
        if self.task_id == 0:
            return self.base.copy(), (bf16_bits(self.base) if shadow else None)
        return apply_ref(self.base, self.delta(), scaling, shadow)
