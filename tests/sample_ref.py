"""Numpy / fp64 restatement of the token sampler (csrc/sample.hip), shared by tools/gen_sample_golden.py and the sampling tests:
Philox4x32-10, the logit recipes of the kernel cases, the kept set by value thresholds and the inverse CDF in ascending token id."""
import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Random123): ``counter`` = 4 and ``key`` = 2 broadcastable arrays of 32-bit words -> 4 uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK32 for x in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return [x.astype(np.uint32) for x in c]


def uniforms(seed, rows, step):
    """The sampler's uniform numbers for rows 0 .. rows-1 at ``step``: key = halves of ``seed``, counter = (row, step, 0, 0),
    u = ((x0 >> 8) + 0.5) * 2^-24 evaluated in fp32 as the kernel does (the sum has 25 bits: it rounds to nearest even).  -> float64
    array of those fp32 values."""
    x0 = philox4x32_10((np.arange(rows), step, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (((x0 >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)


# ---- kernel cases ----------------------------------------------------------------------------------------------------------------
PARAM_SETS = [(1.0, 0, 1.0, 0.0), (0.7, 0, 1.0, 0.0), (1.0, 8, 1.0, 0.0), (1.3, 0, 0.9, 0.0), (0.8, 50, 0.95, 0.0), (1.0, 0, 1.0, 0.05),
              (1.5, 20, 0.8, 0.02), (1.0, 1, 1.0, 0.0)]   # (temperature, top_k, top_p, min_p)
VOCABS = (512, 50277, 50304)
RECIPES = ("planted", "flat")
ROWS = 5
MARGIN = 5e-4
# The flat recipe at V >= 50 277 fills every bf16 value of its range about seventy times over, so under set 3 (T = 1.3, top_p = 0.9, no
# top-k) the decisions the cut can fall between are one tie group = 7e-4 of mass apart: a two-sided 5e-4 cannot exist there.  Those two
# cases ask for 1e-4 instead, still an order above the rounding of a 50 000-term fp32 cumsum.
MARGIN_ON_THE_BF16_GRID = 1e-4


def case_margin(recipe, V, s):
    return MARGIN_ON_THE_BF16_GRID if (recipe == "flat" and V >= 50277 and s == 3) else MARGIN


def case_logits(recipe, V, seed):
    """fp32 logits [ROWS, V] of one kernel case, every value exactly representable in bf16."""
    rs = np.random.RandomState(seed)
    if recipe == "flat":
        x = rs.randn(ROWS, V)
    else:
        x = -20.0 - 4.0 * rs.rand(ROWS, V)
        for row in range(ROWS):
            ids = rs.permutation(V)[:24]
            x[row, ids] = -(0.37 + 0.05 * row) * np.arange(24) + 0.1 * rs.rand(24)
    return torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).float()


def hf_mask(logits, temperature, top_k, top_p, min_p):
    """Kept mask [R, V] from transformers' own warpers in HF's order: temperature, top-k, top-p, min-p."""
    from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = logits.clone().float()
    if temperature != 1.0:
        s = TemperatureLogitsWarper(float(temperature))(None, s)
    if top_k > 0:
        s = TopKLogitsWarper(top_k=int(top_k))(None, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p=float(top_p))(None, s)
    if min_p > 0.0:
        s = MinPLogitsWarper(min_p=float(min_p))(None, s)
    return torch.isfinite(s)


def kept_by_value(logits, temperature, top_k, top_p, min_p):
    """The sampler's kept set in fp64, one row at a time -> (mask [R, V] bool, margin [R]): ``margin`` is the smallest distance of a
    threshold decision to its cut -- top-p: |mass{z > v} - top_p| over the distinct surviving values v (mass renormalised over the top-k
    survivors); min-p: |(p_i / p_max) / min_p - 1| over the survivors of top-k and top-p, the distance in relative probability (both
    sides round relatively).  (Top-k compares stored values: no rounding.)"""
    z = logits.double().numpy() / float(temperature)
    R, V = z.shape
    mask = np.ones((R, V), dtype=bool)
    margin = np.full(R, np.inf)
    for r in range(R):
        zr = z[r]
        keep = np.isfinite(zr)
        if 0 < top_k < V:
            keep &= zr >= np.sort(zr)[V - top_k]
        if top_p < 1.0:
            vals, inv = np.unique(zr[keep], return_inverse=True)          # ascending distinct values of the survivors
            e = np.exp(zr[keep] - zr.max())
            group = np.bincount(inv, weights=e) / e.sum()
            above = np.concatenate([np.cumsum(group[::-1])[::-1][1:], [0.0]])   # mass strictly above each distinct value
            margin[r] = min(margin[r], float(np.abs(above - top_p).min()))
            zstar = vals[above < top_p].min()
            keep &= zr >= zstar
        if min_p > 0.0:
            ratio = np.exp(zr - zr.max())
            margin[r] = min(margin[r], float(np.abs(ratio[keep] / min_p - 1.0).min()))
            keep &= ratio >= min_p
        mask[r] = keep
    return mask, margin


def cdf(logits_row, temperature, mask_row):
    """fp64 probabilities over the kept set and their inclusive cumulative sums in ascending id -> (p [V], cum [V])."""
    z = np.asarray(logits_row, dtype=np.float64) / float(temperature)
    e = np.where(mask_row, np.exp(z - z[mask_row].max()), 0.0)
    p = e / e.sum()
    return p, np.cumsum(p)


def draw(cum, mask_row, u):
    """First kept id whose inclusive cumulative sum exceeds u; the last kept id when rounding leaves none."""
    hit = np.nonzero(mask_row & (cum > u))[0]
    return int(hit[0]) if hit.size else int(np.nonzero(mask_row)[0][-1])


def pack_mask(mask):
    return np.packbits(np.asarray(mask, dtype=bool), axis=-1)


def unpack_mask(packed, V):
    return np.unpackbits(packed, axis=-1)[..., :V].astype(bool)
