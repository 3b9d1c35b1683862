"""CPU: the fp64 reference of the training attention kernels (tests/attn_train_ref.py)
  * pinned to the oracle's causal attention and to torch.autograd of it;
  * shown to leave room: a plain-torch emulation of the kernels' roundings (bf16 rotated operands, fp32 scores and dP, fp32 exp, bf16
    p / dS, fp32 accumulation in 64-row tile order, bf16 store) stays at or below half the bound on every element of every GPU case;
  * shown to be sharp: every mutation of the guard, applied to the reference on the very inputs the GPU tests run, moves an element of
    the affected row past the bound on every instance it is tried on (in some family, at some hot position) -- or the instance is
    listed in INVISIBLE with the reason and asserted to stay unseen, or the mutation in PARTLY with the reason it cannot show everywhere."""
import dataclasses
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import vlpythia_ref as R
from tests import attn_infer_ref as A
from tests import attn_train_ref as T

F64 = torch.float64
CASES = T.cases()


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ------------------------------------------------------------------------------------------------------------------------------
# pin
# ------------------------------------------------------------------------------------------------------------------------------
def _full_attention(qkv, am_full, cos, sin):
    """The oracle's attention core on an assembled [B,S,H,3,D] sequence under the additive mask (tests/test_attn_infer_ref.py)."""
    B, S, H, _, D = qkv.shape
    x = qkv.reshape(B, S, H, 3 * D).transpose(1, 2)
    q, k, v = x.chunk(3, dim=-1)
    q = R.apply_partial_rotary(q, cos[:S].double(), sin[:S].double())
    k = R.apply_partial_rotary(k, cos[:S].double(), sin[:S].double())
    w = torch.matmul(q, k.transpose(2, 3)) * (D ** -0.5) + R.additive_mask(am_full).double()
    return torch.matmul(F.softmax(w, dim=-1), v).transpose(1, 2), w      # [B,S,H,D], [B,H,S,S]


@pytest.mark.parametrize("D,rot", [(16, 4), (32, 16), (20, 6), (16, 0), (16, 16)])
def test_reference_is_the_oracles_attention_and_its_autograd(D, rot):
    B, P, Tt, H = 3, 4, 8, 2
    S = P + Tt
    cos, sin = T.tables(D, rot, S)
    am = torch.ones(B, Tt, dtype=torch.int64)
    am[1, :3] = 0
    am[2, : Tt - 1] = 0
    am_full = torch.cat([torch.ones(B, P, dtype=torch.int64), am], 1)
    qkv = _randn(B, S, H, 3, D, seed=D + rot).requires_grad_(True)
    dout = _randn(B, S, H, D, seed=D + rot + 1)
    want, w = _full_attention(qkv, am_full, cos, sin)
    causal, pad = T.visibility(S, P, am, B)
    f = T.forward(qkv.detach(), causal, pad, cos, sin)
    out = f["out"].reshape(B, S, H, D)
    assert float((out - want.detach()).abs().max()) <= 1e-12
    assert float((f["lse"] - torch.logsumexp(w.detach(), dim=-1)).abs().max()) <= 1e-12
    (dqkv,) = torch.autograd.grad(want, qkv, dout)
    vis = causal[None] & ~pad[:, None, :]
    r = T.backward(qkv.detach(), out, dout, f["lse"], vis, cos, sin)
    assert float((r["dqkv"] - dqkv).abs().max()) <= 1e-10
    assert float((r["delta"] - torch.einsum("bihd,bihd->bhi", dout, want.detach())).abs().max()) <= 1e-10
    assert float((r["colsum"] - dqkv.reshape(B * S, -1).sum(0)).abs().max()) <= 1e-10
    assert bool((r["dk"][pad] == 0).all()) and bool((r["dv"][pad] == 0).all())


def test_bidirectional_reference_is_plain_softmax_attention():
    B, S, H, D = 2, 9, 2, 16
    cos, sin = T.tables(D, 0, S)
    qkv = _randn(B, S, H, 3, D, seed=5)
    causal, pad = T.visibility(S, S, None, B, causal=False)
    f = T.forward(qkv, causal, pad, cos, sin)
    q, k, v = (qkv[:, :, :, i].transpose(1, 2) for i in range(3))
    w = q @ k.transpose(2, 3) / math.sqrt(D)
    assert float((f["out"].reshape(B, S, H, D) - (F.softmax(w, -1) @ v).transpose(1, 2)).abs().max()) <= 1e-12
    assert float((f["lse"] - torch.logsumexp(w, -1)).abs().max()) <= 1e-12


def test_forward_bound_is_the_inference_frames_formula():
    case = next(c for c in CASES if c.path == "mfma")
    inp = T.build(case, "peaked", 16)
    f = T.forward(inp["qkv"], inp["causal"], inp["pad"], inp["cos"], inp["sin"])
    for path in ("mfma", "exact-row"):
        assert torch.equal(T.out_bound(f, path, torch.bfloat16), A.bound(f, path, torch.bfloat16))
    assert "resident" not in A.PATHS


def test_cases_reach_every_kernel_and_both_sides_of_every_border():
    assert len({c.id for c in CASES}) == len(CASES)
    assert all(c.B <= 3 and c.H <= 2 for c in CASES)
    assert all(p >= 1 or max(c.pads) == 0 for c in CASES for p in [c.P]), "a padded prompt needs an image key in front"
    assert all(max(c.pads) <= max(0, c.T - 1) for c in CASES)
    assert T.resident_fits(608, 64) and not T.resident_fits(609, 64) and T.resident_fits(288, 128) and not T.resident_fits(289, 128)
    causal = [c for c in CASES if c.causal and c.dtype == "bf16" and not c.exact]
    res = {(c.D, c.S) for c in causal if c.path == "resident"}
    tiled = {(c.D, c.S, c.variant) for c in causal if c.path == "mfma"}
    assert {(64, s) for s in (7, 33, 64, 65, 129, 288, 608)} | {(128, 40), (128, 257), (128, 288)} <= res
    assert {(64, 609, 0), (64, 641, 0), (128, 289, 0), (256, 14, 0), (256, 83, 0), (256, 288, 0)} <= tiled
    assert {(64, 65, 1), (64, 288, 1), (128, 65, 1), (128, 288, 1)} <= tiled
    assert {(c.P, c.T) for c in causal if c.D == 64} >= {(63, 70), (64, 70), (65, 70), (0, 70), (128, 1), (256, 32)}
    assert {c.rotary for c in causal if c.path != "exact-row"} == {0, 16, 32, 64} and any(c.rotary == c.D for c in causal)
    assert {c.rotary for c in causal if c.path == "resident"} == {0, 16, 32} and {(64, 81, 0), (128, 40, 0)} <= tiled      # rot = 64: tiled
    assert not T.resident_fits(81, 64, 64) and T.resident_fits(81, 64, 32)
    assert {(c.D, c.rotary) for c in causal if c.path == "exact-row"} == {(64, 20), (80, 20)}
    assert {c.D for c in CASES if c.causal and c.dtype == "f32"} == {64, 80, 256}
    assert {(c.dtype, c.D, c.S) for c in CASES if c.op == "bidir"} == {("bf16", 64, 40), ("bf16", 64, 128), ("bf16", 64, 257), ("f32", 64, 40), ("f32", 80, 33)}
    assert all(c.backward == (c.op == "causal" and not c.exact) for c in CASES)


# ------------------------------------------------------------------------------------------------------------------------------
# headroom: the kernels' roundings in plain torch
# ------------------------------------------------------------------------------------------------------------------------------
F32, BF = torch.float32, torch.bfloat16


def _low(x, lowp):
    """an MFMA operand: rounded to bf16 (kept in fp32 for the product); the row kernels keep fp32"""
    return x.to(BF).float() if lowp else x


def _rot32(x, cos, sin, inverse=False):
    """x [B,S,H,D] fp32 rotated for the row's position in fp32 (x c -+ y s)"""
    rot = cos.shape[1]
    if rot == 0:
        return x
    half = rot // 2
    S = x.shape[1]
    c, s = cos[:S, None, :half].float(), sin[:S, None, :half].float()
    if inverse:
        s = -s
    a, b = x[..., :half], x[..., half:rot]
    return torch.cat([a * c - b * s, b * c + a * s, x[..., rot:]], dim=-1)


def emulate_forward(case, inp, store=True):
    """tiled online softmax over 64-key tiles in fp32 with the path's bf16 roundings -> out [B,S,H,D], lse [B,H,S] (fp64 of the stored)"""
    lowp = case.path != "exact-row"
    dt = A.DTYPES[case.dtype]
    qkv = inp["qkv"].float()
    B, S, H, _, D = qkv.shape
    qr, kr, v = _low(_rot32(qkv[:, :, :, 0], inp["cos"], inp["sin"]), lowp), _low(_rot32(qkv[:, :, :, 1], inp["cos"], inp["sin"]), lowp), qkv[:, :, :, 2]
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=F32)
    vis = inp["vis"][:, None]
    m = torch.full((B, H, S), -math.inf, dtype=F32)
    l = torch.zeros(B, H, S, dtype=F32)
    o = torch.zeros(B, H, S, D, dtype=F32)
    for t0 in range(0, S, 64):
        sl = slice(t0, min(S, t0 + 64))
        s = torch.einsum("bihd,bjhd->bhij", qr, kr[:, sl]) * scale
        s = s.masked_fill(~vis[..., sl], -math.inf)
        mn = torch.maximum(m, s.amax(dim=-1))
        alpha = torch.where(mn == -math.inf, torch.zeros((), dtype=F32), (m - mn).exp())
        p = torch.where(s == -math.inf, torch.zeros((), dtype=F32), (s - mn[..., None]).exp())
        p = _low(p, lowp)
        l = l * alpha + p.sum(dim=-1)
        o = o * alpha[..., None] + torch.einsum("bhij,bjhd->bhid", p, v[:, sl])
        m = mn
    out = (o / l[..., None]).transpose(1, 2)
    out = (out.to(dt) if store else out).double()          # store = False: the fp32 value in front of the store
    return out, (m + l.log()).double()


def emulate_backward(case, inp, out, lse, store=True):
    """dq in 64-key tile order, dk / dv in 64-query tile order, fp32 with the path's bf16 roundings -> dq, dk, dv, delta (fp64 of the stored)"""
    lowp = case.path != "exact-row"
    dt = A.DTYPES[case.dtype]
    qkv, do, o, L = inp["qkv"].float(), inp["dout"].float(), out.float(), lse.float()
    B, S, H, _, D = qkv.shape
    cos, sin = inp["cos"], inp["sin"]
    qr, kr, v = _low(_rot32(qkv[:, :, :, 0], cos, sin), lowp), _low(_rot32(qkv[:, :, :, 1], cos, sin), lowp), qkv[:, :, :, 2]
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=F32)
    delta = torch.einsum("bihd,bihd->bhi", do, o)
    s = torch.einsum("bihd,bjhd->bhij", qr, kr) * scale
    p = torch.where(inp["vis"][:, None], (s - L[..., None]).exp(), torch.zeros((), dtype=F32))
    ds = p * (torch.einsum("bihd,bjhd->bhij", do, v) - delta[..., None]) * scale
    p, ds = _low(p, lowp), _low(ds, lowp)
    dq = torch.zeros(B, S, H, D, dtype=F32)
    dk, dv = torch.zeros_like(dq), torch.zeros_like(dq)
    for t0 in range(0, S, 64):
        sl = slice(t0, min(S, t0 + 64))
        dq = dq + torch.einsum("bhij,bjhd->bihd", ds[..., sl], kr[:, sl])
        dk = dk + torch.einsum("bhij,bihd->bjhd", ds[:, :, sl], qr[:, sl])
        dv = dv + torch.einsum("bhij,bihd->bjhd", p[:, :, sl], do[:, sl])
    st = lambda x: (x.to(dt) if store else x).double()
    return st(_rot32(dq, cos, sin, inverse=True)), st(_rot32(dk, cos, sin, inverse=True)), st(dv), delta.double()


def _worst(got, ref, bnd):
    """worst err / bound; an element whose bound is 0 has to be exact"""
    err = (got - ref).abs()
    zero = bnd == 0
    assert bool((err[zero] == 0).all()), "an element with no room is not exact"
    x = float((err[~zero] / bnd[~zero]).max()) if bool((~zero).any()) else 0.0
    assert x == x, "a NaN among the ratios"
    return x


HEADROOM = [(c, f) for c in CASES for f in T.FAMILIES]


@pytest.mark.parametrize("case,fam", HEADROOM, ids=[f"{c.id}-{f}" for c, f in HEADROOM])
def test_the_emulated_roundings_stay_below_half_the_bound(case, fam):
    """err <= bound / 2 on every element.  The bf16 row kernels (exact-row on bf16 data) compute in fp32 and round once, on the store:
    that rounding alone is worth the bound's half ulp, and the fp32 terms beside it are a hundred times smaller, so a correctly
    rounded result already sits at 0.99 of the bound.  There the derived part is held to half instead: the emulation's fp32 value in
    front of the store stays within (bound - ulp) / 2, exactly equal where that is 0 (padded keys, the zeros of census rows), and the
    stored value within the bound."""
    dt = A.DTYPES[case.dtype]
    row_bf16 = case.path == "exact-row" and case.dtype == "bf16"
    B, S, H, D = case.B, case.S, case.H, case.D
    worst = {}

    def note(k, x):
        assert x == x, f"{k}: NaN"
        worst[k] = max(worst.get(k, 0.0), x)

    for hot in T.variants(case, fam):
        inp = T.build(case, fam, hot)
        f = T.forward(inp["qkv"], inp["causal"], inp["pad"], inp["cos"], inp["sin"])
        ob = T.out_bound(f, case.path, dt)
        out_e, lse_e = emulate_forward(case, inp)
        note("lse", _worst(lse_e, f["lse"], T.lse_bound(f, case.path)))
        if row_bf16:
            note("out (stored, of the whole bound)", _worst(out_e.reshape(B * S, H, D), f["out"], 2 * ob))
            note("out", _worst(emulate_forward(case, inp, store=False)[0].reshape(B * S, H, D), f["out"], ob - T.ulp_out(f["out"], dt)))
        else:
            note("out", _worst(out_e.reshape(B * S, H, D), f["out"], ob))
        if case.backward:
            out, lse = T.handed_over(case, f)
            r = T.backward(inp["qkv"], out, inp["dout"], lse, inp["vis"], inp["cos"], inp["sin"])
            bnd = T.backward_bound(inp["qkv"], out, inp["dout"], lse, inp["vis"], inp["cos"], inp["sin"], r, case.path, dt)
            got = dict(zip(("dq", "dk", "dv", "delta"), emulate_backward(case, inp, out, lse)))
            raw = dict(zip(("dq", "dk", "dv", "delta"), emulate_backward(case, inp, out, lse, store=False))) if row_bf16 else {}
            for k in got:
                if row_bf16 and k != "delta":
                    note(k + " (stored, of the whole bound)", _worst(got[k], r[k], 2 * bnd[k]))
                    note(k, _worst(raw[k], r[k], bnd[k] - T.ulp_out(r[k], dt)))
                else:
                    note(k, _worst(got[k], r[k], bnd[k]))
    print(f"[attn-train] emulation {case.label} {fam} {case.id}: worst err / bound = " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    assert all(x <= 0.5 for x in worst.values()), f"{case.id} {fam}: the emulated roundings reach {worst} of the bound"


# ------------------------------------------------------------------------------------------------------------------------------
# guard
# ------------------------------------------------------------------------------------------------------------------------------
GUARD_FAMILIES = ("census", "masked-max", "peaked", "ascending", "descending", "gentle")

# Every mutation has to be seen -- an element of the affected row past its bound -- on EVERY instance it is tried on, in some family and at
# some hot position (the union over GUARD_FAMILIES and the variants of a case).  For a key dropped from a dQ sum the instances are the
# edge rows (some edge key of the row shows), for a query dropped from a dK / dV sum the edge keys.  Two kinds of exception, both named:
#   PARTLY     the mutation cannot show on every instance by its nature; it has to show somewhere, and the log line says where not;
#   INVISIBLE  (case id, mutation) -> the instances (sample, row or key) on which it is not seen; they are asserted to stay unseen.
PARTLY = {
    "fwd: lse of row i+-1": "neighbouring rows of a long sequence have lse values closer than the bound of lse (ascending: 60 / (S - 1) a row)",
    "bwd: lse of row i+-1": "as in the forward: p changes by exp(lse_i - lse_i+-1), which is within e_p where the two are close",
    "bwd: key dropped from dQ": "pair by pair: where one key dominates a row its dS vanishes (p -> 1: dP - delta -> 0), where many share it "
                                "one term is below 4 * 2 * 2^-8 of their sum; the rows are asserted under '[rows]'",
    "bwd: query dropped from dK": "pair by pair, as for dQ; the keys are asserted under '[keys]'",
    "bwd: query dropped from dV": "pair by pair: one of several hundred near-equal p_ij dout_i; the keys are asserted under '[keys]'",
    "bwd: dk of key j+-1": "neighbouring early keys of a long sequence receive the same gradient to within the bound (every later row reaches both)",
    "bwd: dk un-rotated at +-1": "a dk row that is small against its bound on the rotary dims (early keys under the ascending ramp) turns by less than it",
    "bwd: dk with the forward rotation": "as for the un-rotation at +-1",
    "bwd: dq un-rotated at +-1": "a padded query row whose dq is small against its bound on the rotary dims",
}
_PADDED_ROW = "a padded query row: its census dout column meets no visible key's v (dS = 0), and in the other families one term is below the row's bound"
_EARLY_KEY = ("an early key that several hundred queries reach with near-equal weight: one of them, the hot one included, is below "
              "4 * 2 * 2^-8 of the sum over all of them")
WHY = {"bwd: key dropped from dQ [rows]": _PADDED_ROW, "bwd: query dropped from dK [keys]": _EARLY_KEY}      # the reason of every entry below
INVISIBLE = {
    ("causal-bf16-D64r16-B3H2-S288T32", "bwd: query dropped from dK [keys]"): [(2, 65)],
    ("causal-bf16-D64r16-B2H1-S608T40", "bwd: query dropped from dK [keys]"): [(0, 64), (0, 65), (1, 64), (1, 65)],
    ("causal-bf16-D128r32-B2H1-S257T20", "bwd: query dropped from dK [keys]"): [(0, 65), (1, 65)],
    ("causal-bf16-D128r32-B2H1-S288T32", "bwd: query dropped from dK [keys]"): [(1, 64)],
    ("causal-bf16-D64r16-B2H1-S609T40", "bwd: query dropped from dK [keys]"): [(0, 64), (0, 65), (1, 64), (1, 65)],
    ("causal-bf16-D64r16-B2H1-S641T70", "bwd: query dropped from dK [keys]"): [(0, 64), (0, 65), (1, 64), (1, 65)],
    ("causal-bf16-D128r32-B2H1-S289T33", "bwd: query dropped from dK [keys]"): [(1, 64)],
    ("causal-bf16-D128r32-B3H1-S65T10-tiled", "bwd: key dropped from dQ [rows]"): [(2, 60)],
    ("causal-bf16-D128r32-B2H1-S288T32-tiled", "bwd: query dropped from dK [keys]"): [(1, 64)],
}
assert all(name in WHY for _, name in INVISIBLE)


def _unseen(case, t):
    """mutation -> (instances on which it was tried and never seen [(sample, row or key) or (sample, row, key)], instances tried)"""
    out = {}
    for name, calls in t.m.items():
        local = calls[0][1].dim() == 2 and len(calls) == case.B and calls[0][1].shape[0] == len(_edges(case, 0))
        u, k = [], 0
        for ci, (s, o) in enumerate(calls):
            if local:
                e = _edges(case, ci)
                u += [(ci, e[i], e[j]) for i, j in (o & ~s).nonzero().tolist()]
            else:
                u += [tuple(ix) for ix in (o & ~s).nonzero().tolist()]
            k += int(o.sum())
        out[name] = (u, k)
        dim = 1 if "dropped from dQ" in name else (0 if "dropped from d" in name else None)
        if dim is not None:
            u, k = [], 0
            for ci, (s, o) in enumerate(calls):
                e = _edges(case, ci)
                tried, seen = o.any(dim=dim), s.any(dim=dim)
                u += [(ci, e[i]) for i in (tried & ~seen).nonzero().flatten().tolist()]
                k += int(tried.sum())
            out[name + (" [rows]" if dim == 1 else " [keys]")] = (u, k)
    return out


def _edges(case, b):
    """the rows / keys the local mutations are tried on: every edge the kernels have"""
    S, P = case.S, case.P
    e = {0, 1, 15, 16, 17, 63, 64, 65, S - 1, S - 2}            # an edge, and the row behind it: the first query that can be dropped from its key
    if case.causal:
        e |= {P - 1, P, P + 1, P + case.pads[b], P + case.pads[b] + 1, (P + S) // 2}
    return sorted(j for j in e if 0 <= j < S)


class _Tally:
    """Per mutation, the instances it was tried on (rows, keys or (row, key) pairs: boolean masks in call order) and those on which an
    element moved past its bound -- the union over the families and the hot positions of a case."""

    def __init__(self):
        self.m, self.idx = {}, {}

    def begin(self):
        self.idx = {}

    def add(self, name, seen, ok):
        i = self.idx.get(name, 0)
        self.idx[name] = i + 1
        lst = self.m.setdefault(name, [])
        if i == len(lst):
            lst.append([seen & ok, ok.clone()])
        else:
            assert torch.equal(lst[i][1], ok), name
            lst[i][0] |= seen & ok

    def rows(self, name, a, b, bnd, rows):
        """a, b, bnd [..., H, D] with leading dims matching rows (bool): the affected rows; a row is seen if an element of it, in any
        head, differs by more than its bound"""
        self.add(name, ((a - b).abs() > bnd).any(dim=-1).any(dim=-1), rows)

    def counts(self, name, dim=None):
        """(seen, tried); dim: a (row, key) pair mask reduced to the rows (1) or the keys (0) that have a tried pair"""
        red = (lambda x: x) if dim is None else (lambda x: x.any(dim=dim))
        return sum(int(red(s).sum()) for s, _ in self.m[name]), sum(int(red(o).sum()) for _, o in self.m[name])


def _guard_forward(case, inp, f, dt, t):
    B, S, H, D = case.B, case.S, case.H, case.D
    cos, sin = inp["cos"], inp["sin"]
    causal, pad, vis = inp["causal"], inp["pad"], inp["vis"]
    out, bnd = f["out"].reshape(B, S, H, D), T.out_bound(f, case.path, dt).reshape(B, S, H, D)
    nk = f["nk"].reshape(B, S)
    gs = T.groups(inp["qkv"], causal, pad)

    def again(name, rows, gs2):
        t.rows(name, T.forward_of(gs2, cos, sin)["out"].reshape(B, S, H, D), out, bnd, rows)

    # a key dropped from one row: (out_i - p_ij v_j) / (1 - p_ij), on the edges
    for b in range(B):
        res, e = f["res"][b], torch.tensor(_edges(case, b))
        p = res["p"][:, e][:, :, e]                                                 # [H,E,E]
        v = inp["qkv"][b, e, :, 2].transpose(0, 1)                                  # [H,E,D]
        o = out[b, e].transpose(0, 1)                                               # [H,E,D]
        mut = (o[:, :, None, :] - p[..., None] * v[:, None, :, :]) / (1.0 - p).clamp(min=1e-300)[..., None]
        seen = ((mut - o[:, :, None, :]).abs() > bnd[b, e].transpose(0, 1)[:, :, None, :]).any(dim=-1).any(dim=0)      # [E,E]
        ok = vis[b][e][:, e] & (nk[b, e] > 1)[:, None]
        t.add("fwd: key dropped", seen, ok)
    if case.causal:
        nxt = torch.zeros(B, S, dtype=torch.bool)
        nxt[:, :-1] = ~pad[:, 1:]
        again("fwd: key i+1 visible", nxt, T.groups(inp["qkv"], torch.tril(torch.ones(S, S, dtype=torch.bool), 1), pad))
        rows = (nk > 1) & ~pad
        c2 = torch.tril(torch.ones(S, S, dtype=torch.bool), -1)
        c2[0, 0] = True
        again("fwd: key i hidden", rows & (torch.arange(S) > 0)[None], T.groups(inp["qkv"], c2, pad))
        if bool(pad.any()):
            again("fwd: padded key visible", (causal[None] & pad[:, None, :]).any(dim=2), T.groups(inp["qkv"], causal, torch.zeros_like(pad)))
        if case.T > 0:
            pad2 = pad.clone()
            first = torch.tensor([case.P + case.pads[b] for b in range(B)])
            pad2[torch.arange(B), first] = True
            rows = (torch.arange(S)[None] >= first[:, None]) & (case.P > 0)
            if case.P > 0:
                again("fwd: first text key hidden", rows, T.groups(inp["qkv"], causal, pad2))
        if len(set(case.pads)) > 1:
            for o in (1, -1):
                pad2 = torch.roll(pad, o, dims=0)
                again("fwd: mask of sample b+-1", ((pad2 != pad)[:, None, :] & causal[None]).any(dim=2), T.groups(inp["qkv"], causal, pad2))
    if case.rotary > 0:
        for o in (1, -1):
            again("fwd: q rotated at +-1", nk > 1, [dataclasses.replace(g, qpos=g.qpos + o) for g in gs])
            again("fwd: k rotated at +-1", nk > 1, [dataclasses.replace(g, kpos=g.kpos + o) for g in gs])
    lb = T.lse_bound(f, case.path)
    for o in (1, -1):
        seen = (torch.roll(f["lse"], o, dims=2) - f["lse"]).abs() > lb
        t.add("fwd: lse of row i+-1", seen, torch.ones_like(seen))


def _guard_backward(case, inp, f, dt, t):
    B, S, H, D = case.B, case.S, case.H, case.D
    cos, sin, vis, pad = inp["cos"], inp["sin"], inp["vis"], inp["pad"]
    out, lse = T.handed_over(case, f)
    args = (inp["qkv"], out, inp["dout"], lse, vis, cos, sin)
    r = T.backward(*args)
    bnd = T.backward_bound(*args, r, case.path, dt)
    rs = 1.0 / math.sqrt(D)
    every = torch.ones(B, S, dtype=torch.bool)
    multi = vis.sum(dim=2) > 1           # a row with one visible key has dS = 0 (dP = delta): its dq is 0 whatever is done to dS

    def moved(name, r2, keys=("dq", "dk", "dv"), rows=every):
        seen = torch.zeros(B, S, dtype=torch.bool)
        for k in keys:
            seen |= ((r2[k] - r[k]).abs() > bnd[k]).any(dim=-1).any(dim=-1)
        t.add(name, seen, rows)

    for b in range(B):
        e = torch.tensor(_edges(case, b))
        ok = vis[b][e][:, e]                                                        # [E(i),E(j)]
        okq = ok & multi[b, e][:, None]
        dS = r["dS"][b][:, e][:, :, e]                                              # [H,E,E]
        p = r["p"][b][:, e][:, :, e]
        # key j dropped from row i's dQ sum: dq_i loses unrot_i(dS_ij k~_j / sqrt D)
        term = dS.permute(1, 2, 0)[..., None] * r["kr"][b, e][None] * rs             # [E(i),E(j),H,D]
        term = torch.stack([T._rotate(term[a], e[a].expand(len(e)), cos, sin, inverse=True) for a in range(len(e))])
        seen = (term.abs() > bnd["dq"][b, e][:, None]).any(dim=-1).any(dim=-1)
        t.add("bwd: key dropped from dQ", seen, okq)
        # query i dropped from key j's sums: dv_j loses p_ij dout_i, dk_j loses unrot_j(dS_ij q~_i / sqrt D)
        tv = p.permute(1, 2, 0)[..., None] * inp["dout"][b, e][:, None]             # [E(i),E(j),H,D]
        seen = (tv.abs() > bnd["dv"][b, e][None]).any(dim=-1).any(dim=-1)
        t.add("bwd: query dropped from dV", seen, ok)
        tk = dS.permute(1, 2, 0)[..., None] * r["qr"][b, e][:, None] * rs
        tk = torch.stack([T._rotate(tk[:, a], e[a].expand(len(e)), cos, sin, inverse=True) for a in range(len(e))], dim=1)
        seen = (tk.abs() > bnd["dk"][b, e][None]).any(dim=-1).any(dim=-1)
        t.add("bwd: query dropped from dK", seen, okq)
        diag = torch.eye(len(e), dtype=torch.bool) & ok
        t.add("bwd: diagonal query dropped from dK / dV", ((tk.abs() > bnd["dk"][b, e][None]) | (tv.abs() > bnd["dv"][b, e][None])).any(dim=-1).any(dim=-1), diag)
    for o in (1, -1):
        moved("bwd: delta of row i+-1", T.backward(*args, delta=torch.roll(r["delta"], o, dims=2)), ("dq",))
        a2 = list(args)
        a2[3] = torch.roll(lse, o, dims=2)
        moved("bwd: lse of row i+-1", T.backward(*a2), ("dq",))
        if case.rotary > 0:
            r2 = T.backward(*args, unrot_shift=o)
            moved("bwd: dq un-rotated at +-1", r2, ("dq",), multi)
            moved("bwd: dk un-rotated at +-1", r2, ("dk",), ~pad)
        for k in ("dk", "dv"):
            keep = torch.ones(B, S, dtype=torch.bool)
            keep[:, 0 if o == 1 else -1] = False
            keep &= ~(pad & torch.roll(pad, o, dims=1))      # two padded keys: zeros for zeros
            moved(f"bwd: {k} of key j+-1", {k: torch.roll(r[k], o, dims=1)}, (k,), keep)
    if case.rotary > 0:
        r2 = T.backward(*args, unrot_forward=True)
        moved("bwd: dq with the forward rotation", r2, ("dq",), torch.arange(S)[None].expand(B, S) > 0)
        moved("bwd: dk with the forward rotation", r2, ("dk",), (torch.arange(S)[None].expand(B, S) > 0) & ~pad)
    r2 = T.backward(*args, ds_scale=False)
    moved("bwd: dS without 1 / sqrt D", r2, ("dq",), multi)
    moved("bwd: dS without 1 / sqrt D (dk)", r2, ("dk",), ~pad)
    if bool(pad.any()):
        a2 = list(args)
        a2[4] = inp["causal"][None].expand(B, S, S)
        r2 = T.backward(*a2)
        got = ((r2["dk"] != 0) | (r2["dv"] != 0)).any(dim=-1).any(dim=-1)           # the GPU test asserts exact zeros there
        t.add("bwd: padded key receives gradient", got, pad)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_the_bounds_see_every_mutation(case):
    dt = A.DTYPES[case.dtype]
    t = _Tally()
    for fam in GUARD_FAMILIES:
        for hot in T.variants(case, fam):
            inp = T.build(case, fam, hot)
            f = T.forward(inp["qkv"], inp["causal"], inp["pad"], inp["cos"], inp["sin"])
            t.begin()
            _guard_forward(case, inp, f, dt, t)
            if case.backward:
                _guard_backward(case, inp, f, dt, t)
    unseen = _unseen(case, t)
    print(f"[attn-train] guard {case.id}: " + "; ".join(f"{n} {len(u)}/{k} unseen" for n, (u, k) in sorted(unseen.items())))
    want = {"fwd: key dropped", "fwd: lse of row i+-1"}
    if case.causal:
        want |= {"fwd: key i+1 visible", "fwd: key i hidden"}
    if case.backward:
        want |= {"bwd: key dropped from dQ [rows]", "bwd: query dropped from dV [keys]", "bwd: query dropped from dK [keys]", "bwd: delta of row i+-1",
                 "bwd: lse of row i+-1", "bwd: dS without 1 / sqrt D", "bwd: dk of key j+-1", "bwd: dv of key j+-1"}
    assert want <= {n for n, (_, k) in unseen.items() if k}, f"{case.id}: nothing tried for {want - set(unseen)}"
    listed = {n: INVISIBLE[(cid, n)] for (cid, n) in INVISIBLE if cid == case.id}
    assert set(listed) <= set(unseen) and not set(listed) & set(PARTLY)
    for name, (u, k) in unseen.items():
        if name in PARTLY:
            assert len(u) < k, f"{case.id}: {name} is seen nowhere"
        else:
            assert set(u) == set(listed.get(name, ())), (f"{case.id}: {name}: unseen at {sorted(u)}, listed as invisible at "
                                                         f"{sorted(listed.get(name, ()))}")
    assert 4 * len(listed) <= len(unseen), f"{case.id}: {len(listed)} of {len(unseen)} mutations have invisible instances"
