"""CPU: the fp64 reference of the inference attention kernels (tests/attn_infer_ref.py) pinned to the oracle's full causal attention,
and the guard that the bound of tests/test_gpu_attn_infer_oracle.py can see the mistakes it is there for: every mutation below, applied
to the reference on the very inputs the GPU tests run, moves at least one element of the affected row by more than the bound."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from oracle import vlpythia_ref as R
from tests import attn_infer_ref as A

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------------------------
# pin: each function equals the matching rows of the oracle's attention on the assembled sequence
# ------------------------------------------------------------------------------------------------------------------------------
def _full_attention(qkv, am_full, cos, sin):
    """The oracle's attention core on an assembled [B,S,H,3,D] sequence under the additive mask (tests/test_gpu_kernels.py, _attn_ref)."""
    B, S, H, _, D = qkv.shape
    x = qkv.reshape(B, S, H, 3 * D).transpose(1, 2)
    q, k, v = x.chunk(3, dim=-1)
    q = R.apply_partial_rotary(q, cos[:S].double(), sin[:S].double())
    k = R.apply_partial_rotary(k, cos[:S].double(), sin[:S].double())
    w = torch.matmul(q, k.transpose(2, 3)) * (D ** -0.5) + R.additive_mask(am_full).double()
    return torch.matmul(F.softmax(w, dim=-1), v).transpose(1, 2)      # [B,S,H,D]


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def _mask(B, T, pads):
    am = torch.ones(B, T, dtype=torch.int64)
    for b, p in enumerate(pads):
        am[b, :p] = 0
    return am


def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-12, float((a - b).abs().max())


@pytest.mark.parametrize("prerot", [False, True])
@pytest.mark.parametrize("D,rot", [(16, 4), (32, 16), (20, 6)])
def test_decode_is_the_last_row_of_the_oracle(D, rot, prerot):
    B, P, T, H, cap, t = 3, 3, 4, 2, 3, 2
    S0, S = P + T, P + T + t + 1
    cos, sin = A.tables(D, rot, S0 + cap)
    am = _mask(B, T, (0, 2, T))                     # no padding, left padding, an all-padding prompt
    seq = _randn(B, S, H, 3, D, seed=D + rot)
    want = _full_attention(seq, torch.cat([torch.ones(B, P, dtype=torch.int64), am, torch.ones(B, t + 1, dtype=torch.int64)], 1), cos, sin)[:, -1]
    cache = A.rotate_k(seq, S, H, D, rot, cos, sin) if prerot else seq
    new = torch.zeros(B, cap, H, 3, D, dtype=F64)
    new[:, :t] = cache[:, S0:S0 + t]
    new[:, t] = seq[:, S0 + t]
    got = A.decode(cache[:, :S0], new, t, am, P, rot, cos, sin, prerot)
    _close(got["out"], want)
    assert got["nk"].tolist() == [S, S - 2, S - T]
    if prerot:
        _close(got["k_t"], A.rotate_k(seq, S, H, D, rot, cos, sin)[:, S0 + t, :, 1])


def test_decode_beam_is_the_last_row_of_the_oracle_on_each_beams_history():
    B, k, P, T, H, D, rot, cap, t = 2, 3, 3, 4, 2, 16, 4, 4, 3
    S0, S = P + T, P + T + t + 1
    cos, sin = A.tables(D, rot, S0 + cap)
    am = _mask(B, T, (1, T))
    prefix = _randn(B, S0, H, 3, D, seed=1)
    slots = _randn(B * k, cap, H, 3, D, seed=2)            # un-rotated rows of every slot
    anc = torch.tensor([[1, 2, 0, 0], [1, 1, 1, 1], [2, 0, 1, 2], [5, 3, 4, 3], [3, 3, 5, 4], [4, 5, 3, 5]], dtype=torch.int32)   # reordered
    new = A.rotate_k(slots, cap, H, D, rot, cos[S0:], sin[S0:])
    new[:, t] = slots[:, t]
    got = A.decode_beam(A.rotate_k(prefix, S0, H, D, rot, cos, sin), new, anc, t, k, am, P, rot, cos, sin)
    hist = torch.stack([torch.stack([slots[int(anc[r, j]), j] for j in range(t)] + [slots[r, t]]) for r in range(B * k)])
    seq = torch.cat([prefix.repeat_interleave(k, dim=0), hist], dim=1)
    am_full = torch.cat([torch.ones(B, P, dtype=torch.int64), am, torch.ones(B, t + 1, dtype=torch.int64)], 1).repeat_interleave(k, dim=0)
    _close(got["out"], _full_attention(seq, am_full, cos, sin)[:, -1])


def test_suffix_is_the_text_rows_of_the_oracle():
    B, N, P, T, H, D, rot = 3, 3, 3, 5, 2, 16, 4
    cos, sin = A.tables(D, rot, P + T)
    am = _mask(B, T, (0, 2, T))                     # prompt 1: padded query rows; prompt 2: all padding
    img, txt = _randn(N, P, H, 3, D, seed=3), _randn(B, T, H, 3, D, seed=4)
    index = torch.tensor([2, 0, 2])                 # unsorted, image 1 unused
    got = A.suffix(img, index, txt, am, rot, cos, sin)
    seq = torch.cat([img[index], txt], dim=1)
    want = _full_attention(seq, torch.cat([torch.ones(B, P, dtype=torch.int64), am], 1), cos, sin)[:, P:]
    _close(got["out"], want.reshape(B * T, H, D))
    assert got["nk"].view(B, T)[1].tolist() == [P, P, P + 1, P + 2, P + 3] and got["nk"].view(B, T)[2].tolist() == [P] * T


def test_cand_is_the_candidate_rows_of_the_oracle_and_candidates_do_not_see_each_other():
    B, C, Acand, P, T, H, D, rot = 2, 3, 4, 3, 4, 2, 16, 4
    S0 = P + T
    cos, sin = A.tables(D, rot, S0 + Acand)
    am = _mask(B, T, (0, 3))
    pre, cnd = _randn(B, S0, H, 3, D, seed=5), _randn(B, C, Acand, H, 3, D, seed=6)
    got = A.cand(pre, cnd, am, rot, cos, sin)
    seq = torch.cat([pre[:, None].expand(B, C, S0, H, 3, D), cnd], dim=2).reshape(B * C, S0 + Acand, H, 3, D)
    am_full = torch.cat([torch.ones(B, P, dtype=torch.int64), am, torch.ones(B, Acand, dtype=torch.int64)], 1).repeat_interleave(C, dim=0)
    _close(got["out"], _full_attention(seq, am_full, cos, sin)[:, S0:].reshape(B * C * Acand, H, D))
    other = cnd.clone()
    other[:, 1] = _randn(B, Acand, H, 3, D, seed=7)                  # isolation: candidate 1 changes, candidates 0 and 2 do not move
    moved = (A.cand(pre, other, am, rot, cos, sin)["out"] - got["out"]).abs().reshape(B, C, -1).amax(dim=-1)
    assert bool((moved[:, 1] > 0).all()) and float(moved[:, 0].max()) == 0.0 and float(moved[:, 2].max()) == 0.0
    none = A.cand(pre, cnd, None, rot, cos, sin)                     # T = 0: no mask
    _close(none["out"], A.cand(pre, cnd, torch.ones(B, T, dtype=torch.int64), rot, cos, sin)["out"])


def test_rotate_k_is_the_oracle_rotation_of_the_k_third():
    B, S, H, D, rot = 2, 5, 2, 16, 8
    cos, sin = A.tables(D, rot, S)
    x = _randn(B, S, H, 3, D, seed=8)
    got = A.rotate_k(x, S, H, D, rot, cos, sin)
    want = R.apply_partial_rotary(x[:, :, :, 1].transpose(1, 2), cos.double(), sin.double()).transpose(1, 2)
    _close(got[:, :, :, 1], want)
    assert torch.equal(got[:, :, :, 0], x[:, :, :, 0]) and torch.equal(got[:, :, :, 2], x[:, :, :, 2])
    assert bool((A.rotate_k_operands(x, S, H, D, rot, cos, sin) >= got[:, :, :, 1].abs() - 1e-15).all())


def test_ulp_out_is_half_an_ulp():
    x = torch.tensor([1.0, 1.5, 0.75, 3.0, 0.0], dtype=F64)
    assert A.ulp_out(x, torch.bfloat16)[:4].tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 2.0 ** -7]
    assert A.ulp_out(x, torch.float32)[:4].tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -25, 2.0 ** -23]
    assert 0.0 < float(A.ulp_out(x, torch.float32)[4]) < 1e-40


# ------------------------------------------------------------------------------------------------------------------------------
# the case list reaches what it is meant to reach
# ------------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_kernel_and_both_sides_of_every_switch():
    cases = A.all_cases()
    assert len({c.id for c in cases}) == len(cases)
    assert all(c.B <= 3 and c.H <= 2 for c in cases)
    dec = [c for c in cases if c.op == "decode"]
    assert {c.path for c in dec} == {"scalar", "fused", "fused-prerot", "flat"}
    assert {(c.D, c.rotary) for c in dec if c.path == "scalar"} == {(64, 20), (80, 20)}
    nk = lambda c: c.S0 + c.t + 1
    flat_side = {(c.D, nk(c)) for c in dec if c.path == "flat"}
    fused_side = {(c.D, nk(c)) for c in dec if c.path == "fused-prerot" and c.dtype == "bf16" and c.flat}
    assert {(64, 768), (128, 384)} <= flat_side and {(64, 769), (128, 385)} <= fused_side
    assert 256 in {c.T for c in dec if c.path == "flat"} and 257 in {c.T for c in dec if c.path == "fused-prerot" and c.dtype == "bf16" and c.flat}
    assert {(c.k, A.beam_kb(c.k)) for c in cases if c.op == "beam"} == {(1, 2), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8)}
    assert {c.path for c in cases if c.op in ("suffix", "cand") and c.dtype == "bf16"} == {"mfma", "exact-row"}


# ------------------------------------------------------------------------------------------------------------------------------
# guard
# ------------------------------------------------------------------------------------------------------------------------------
def _unnormalised(res, v):
    """w = exp(s - m) and O = sum_j w_j v_j of every row, for every key (visible or not): softmax with one key more or less is
    (O +- w_j v_j) / (L +- w_j)."""
    w = (res["s"] - res["m"][..., None]).exp()                          # [H,Rq,nk]
    O = torch.einsum("hrj,jhd->hrd", res["p"], v) * res["L"][..., None]
    return w, O


def _seen(dev, bnd):
    """dev [H,Rq,nk,D] against bnd [Rq,H,D] -> [H,Rq,nk]: some element of the row moved by more than its bound"""
    return (dev.abs() > bnd.transpose(0, 1)[:, :, None, :]).any(dim=-1)


def _drop_each(g, res, bnd):
    """every visible key of every row left out in turn -> the (row, head, key) triples the bound does not see"""
    w, O = _unnormalised(res, g.v)
    vis = g.vis()[None] & (res["nk"] > 1)[None, :, None]                # a row with one key has nothing to drop
    vj = g.v.transpose(0, 1)[:, None]                                   # [H,1,nk,D]
    mut = (O[:, :, None, :] - w[..., None] * vj) / (res["L"][..., None] - w).clamp(min=1e-300)[..., None]
    return int((vis & ~_seen(mut - res["out"].transpose(0, 1)[:, :, None, :], bnd)).sum()), int(vis.sum())


def _include_each(g, res, bnd):
    """every padded key in a row's range let in in turn"""
    w, O = _unnormalised(res, g.v)
    hid = (g.causal & g.pad[None])[None].expand_as(w)
    vj = g.v.transpose(0, 1)[:, None]
    mut = (O[:, :, None, :] + w[..., None] * vj) / (res["L"][..., None] + w)[..., None]
    return int((hid & ~_seen(mut - res["out"].transpose(0, 1)[:, :, None, :], bnd)).sum()), int(hid.sum())


def _row_seen(a, b, bnd, rows):
    """rows [Rq] bool: every (row, head) of them has an element that differs by more than the bound -> (missed, checked)"""
    seen = ((a - b).abs() > bnd).any(dim=-1)                            # [Rq,H]
    return int((~seen[rows]).sum()), int(rows.sum()) * a.shape[1]


def _shortcut_equals_a_recomputation(g, res, cos, sin):
    j = int(g.vis()[-1].nonzero()[0])
    w, O = _unnormalised(res, g.v)
    mut = (O[:, -1] - w[:, -1, j, None] * g.v[j]) / (res["L"][:, -1, None] - w[:, -1, j, None])
    causal = g.causal.clone()
    causal[-1, j] = False
    again = A.solve(dataclasses.replace(g, causal=causal), cos, sin)["out"][-1]
    assert float((mut - again).abs().max()) <= 1e-12


def _hot_index(case, g_index, hot, inp):
    """index of the hot key on the key axis of group g_index, or None if that group does not hold it"""
    S0 = case.S0
    if hot[0] == "key":
        b = {"decode": g_index, "beam": g_index // case.k, "suffix": g_index, "cand": g_index // case.C}[case.op]
        j = A._resolve_hot(case, b, hot[1])
        if case.op == "suffix" and j < case.P <= hot[1]:
            return None                      # an all-padding prompt has no hot text key, and the image store's hot key is not moved for it
        if case.op == "beam" and j >= S0:
            return None
        return j
    if hot[0] == "cand":
        return S0 + hot[2] if g_index % case.C == hot[1] else None
    b, r = g_index // case.k, g_index % case.k      # ("slot", slot, row): the beams that read that row from that slot
    if hot[2] > case.t:
        return None
    named = r if hot[2] == case.t else int(inp["anc"][g_index, hot[2]]) - b * case.k
    return S0 + hot[2] if named == hot[1] else None


GUARD = [(c, f) for c in A.all_cases() for f in ("census", "masked-max", "peaked")]


@pytest.mark.parametrize("case,fam", GUARD, ids=[f"{c.id}-{f}" for c, f in GUARD])
def test_the_bound_sees_every_mutation(case, fam):
    dtype = A.DTYPES[case.dtype]
    missed, checked = {}, {}

    def tally(name, pair):
        missed[name] = missed.get(name, 0) + pair[0]
        checked[name] = checked.get(name, 0) + pair[1]

    for hot in A.variants(case, fam):
        inp = A.build(case, fam, hot)
        cos, sin = inp["cos"], inp["sin"]
        groups = A.groups_of(case, inp)
        for gi, g in enumerate(groups):
            res = A.solve(g, cos, sin)
            bnd = A.bound(res, case.path, dtype)
            if fam == "census":
                tally("drop", _drop_each(g, res, bnd))
                if gi == 0:
                    _shortcut_equals_a_recomputation(g, res, cos, sin)
            if fam in ("census", "masked-max"):
                tally("include", _include_each(g, res, bnd))
            if fam != "peaked":
                continue
            j = _hot_index(case, gi, hot, inp)
            if j is not None and not bool(g.pad[j]):
                rows = g.vis()[:, j] & (res["nk"] > 1)
                for o in (-1, 1):            # V of the neighbouring key in place of the hot key's
                    if 0 <= j + o < len(g.kpos):
                        v = g.v.clone()
                        v[j] = g.v[j + o]
                        tally("v-neighbour", _row_seen(A.solve(dataclasses.replace(g, v=v), cos, sin)["out"], res["out"], bnd, rows))
                for o in (-1, 1):            # the hot key (where the kernel rotates it), then the query, rotated one position off
                    if bool(g.krot[j]) and g.kpos[j] + o >= 0:
                        kpos = g.kpos.clone()
                        kpos[j] += o
                        tally("rotate-key", _row_seen(A.solve(dataclasses.replace(g, kpos=kpos), cos, sin)["out"], res["out"], bnd, rows))
                    tally("rotate-query", _row_seen(A.solve(dataclasses.replace(g, qpos=g.qpos + o), cos, sin)["out"], res["out"], bnd, rows))
            if case.op == "beam" and hot[0] == "slot":
                # generated row j read from the beam's own slot where anc names another: seen wherever exactly one of the two is hot
                k, t, S0 = case.k, case.t, case.S0
                b, r = gi // k, gi % k
                for jrow in range(t):
                    named = int(inp["anc"][gi, jrow]) - b * k
                    if named != r and hot[2] == jrow and (hot[1] == named) != (hot[1] == r):
                        kk, v = g.k.clone(), g.v.clone()
                        kk[S0 + jrow], v[S0 + jrow] = inp["new"][gi, jrow, :, 1], inp["new"][gi, jrow, :, 2]
                        tally("own-slot", _row_seen(A.solve(dataclasses.replace(g, k=kk, v=v), cos, sin)["out"], res["out"], bnd,
                                                    torch.ones(1, dtype=torch.bool)))
            if case.op == "cand" and hot[0] == "cand" and case.C > 1:
                # row hot[2] of another candidate in place of the own one: seen by every row from hot[2] on, in the hot candidate (it loses
                # its hot key) and in the others (they gain one)
                b, c = gi // case.C, gi % case.C
                other = hot[1] if c != hot[1] else (c + 1) % case.C
                kk, v = g.k.clone(), g.v.clone()
                kk[case.S0 + hot[2]], v[case.S0 + hot[2]] = inp["qkv_cand"][b, other, hot[2], :, 1], inp["qkv_cand"][b, other, hot[2], :, 2]
                rows = torch.arange(case.A) >= hot[2]
                tally("other-candidate", _row_seen(A.solve(dataclasses.replace(g, k=kk, v=v), cos, sin)["out"], res["out"], bnd, rows))
    assert all(n == 0 for n in missed.values()), f"{case.id} {fam} ({case.path}): the bound does not see {missed} of {checked}"
    want = set()
    if fam == "census":
        want |= {"drop"}
    if fam == "peaked":
        want |= {"v-neighbour", "rotate-query", "rotate-key"}
        if case.op == "beam" and case.k > 1 and case.t > 0:
            want.add("own-slot")
        if case.op == "cand" and case.C > 1:
            want.add("other-candidate")
    if fam in ("census", "masked-max") and any(0 < p for p in case.pads) and case.T > 0:
        want.add("include")
    assert all(checked.get(name, 0) > 0 for name in want), f"{case.id} {fam}: nothing checked for {want - {n for n, c in checked.items() if c}}"
