"""GPU: the training attention kernels against the fp64 reference of tests/attn_train_ref.py, element by element within the bounds
derived there: out and lse of the forward (``ops.attn_fwd``, ``ops.attn_fwd_exact_bf16``, ``ops.attn_fwd_bidir``), dq, dk, dv and delta
of the backward (``ops.attn_bwd``), its column sums, exact zeros on padded keys, and the same bits with and without ``colsum``.  The
inputs make one wrong key, query, row statistic or rotation visible (census, peaked with the hot key and the hot query on every edge,
ascending / descending, masked-max; one-hot or bit-hash dout rows); tests/test_attn_train_ref.py shows on the CPU that the kernels'
own roundings use at most half of these bounds and that each of the guard's mutations exceeds them.

The backward is checked twice per input: handed the fp64 forward rounded to the dtype (the backward alone), and handed the kernel's
own out and lse with the reference recomputed from those tensors (the coupling the model uses).

Kernel reached by each case (``Case.path`` / ``Case.label``: attn.hip mfma_ok, attn_mfma.hip attn_resident_fits, mafed_attn_set_variant):
  bf16, D = 64, rot in {0, 16, 32}        resident up to S = 608 (8-wave forward, 4-wave backwards), tiled from S = 609 and under variant 1
  bf16, D = 128, rot in {16, 32}          resident up to S = 288, tiled from S = 289 and under variant 1
  bf16, D = 64 / 128, rot = 64            tiled (the resident kernels rotate 32 dims of their column operand at the most)
  bf16, D = 256                           tiled
  bf16, D = 80 or rot = 20; fp32          the exact row kernels
  bidirectional                           bf16 D = 64: the resident forward without the causal test; fp32: the exact row kernel"""
import pytest
import torch

from tests import attn_infer_ref as A
from tests import attn_train_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(c, f) for c in T.cases() for f in T.FAMILIES]


def _dev(x, dtype):
    return x.to(dtype).to(DEV).contiguous()


class _Variant:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from mafed_amd import _lib
        self.lib = _lib.load()
        assert self.lib.mafed_attn_set_variant(self.v) == 0

    def __exit__(self, *exc):
        self.lib.mafed_attn_set_variant(0)


def _forward(case, inp, ops, tabs):
    """-> out [B*S,H,D], lse [B,H,S] on the CPU (kernel dtype / fp32)"""
    dt = A.DTYPES[case.dtype]
    B, S, H, D = case.B, case.S, case.H, case.D
    qkv = _dev(inp["qkv"], dt).view(B * S, -1)
    if case.op == "bidir":
        out = ops.attn_fwd_bidir(qkv, B, S, H, D)
        # attn_fwd_bidir keeps its lse to itself: the same entry point once more with a buffer of ours.  Mirrors include/mafed_hip.h:
        # int mafed_attn_fwd_bidir(const void* qkv, mafed_dtype dtype, int B, int S, int H, int D, void* out, float* lse, void* stream)
        # (argument types are checked through _lib.SIGNATURES when the library is loaded)
        from mafed_amd import _lib
        lse = torch.empty(B, H, S, dtype=torch.float32, device=DEV)
        out2 = torch.empty_like(out)
        ops.check(_lib.load().mafed_attn_fwd_bidir(ops._ptr(qkv), ops._dt(qkv), B, S, H, D, ops._ptr(out2), ops._ptr(lse), ops._stream()), "mafed_attn_fwd_bidir")
        assert torch.equal(out, out2), "a second bidirectional forward gives other bits"
    else:
        fn = ops.attn_fwd_exact_bf16 if case.exact else ops.attn_fwd
        with _Variant(case.variant):
            out, lse = fn(qkv, B, S, H, D, case.rotary, tabs[0], tabs[1], inp["am"].to(DEV))
    assert out.dtype == dt and lse.dtype == torch.float32
    torch.cuda.synchronize()
    return out.cpu().view(B * S, H, D), lse.cpu()


def _backward(case, inp, ops, tabs, out, lse, c0):
    """out [B,S,H,D] / lse [B,H,S] (CPU, the values to hand over) -> dqkv [B,S,H,3,D], delta [B,H,S], colsum after the call from c0"""
    from mafed_amd import _lib
    dt = A.DTYPES[case.dtype]
    B, S, H, D, rot = case.B, case.S, case.H, case.D, case.rotary
    qkv, o, do = _dev(inp["qkv"], dt).view(B * S, -1), _dev(out, dt).view(B * S, -1), _dev(inp["dout"], dt).view(B * S, -1)
    L, am = _dev(lse, torch.float32), inp["am"].to(DEV)
    col = c0.to(DEV).clone()
    with _Variant(case.variant):
        plain = ops.attn_bwd(qkv, o, do, L, B, S, H, D, rot, tabs[0], tabs[1], am)
        summed = ops.attn_bwd(qkv, o, do, L, B, S, H, D, rot, tabs[0], tabs[1], am, colsum=col)
        # ops.attn_bwd keeps delta to itself: the same entry point once more with a buffer of ours.  Mirrors include/mafed_hip.h:
        # int mafed_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, mafed_dtype dtype, int B, int S, int H, int D,
        #                    int rot, const float* rot_cos, const float* rot_sin, const int64_t* attention_mask, int T, void* dqkv, float* delta,
        #                    void* stream)   -- the argument list ops.attn_bwd itself passes
        third, delta = torch.empty_like(qkv), torch.empty(B, H, S, dtype=torch.float32, device=DEV)
        ops.check(_lib.load().mafed_attn_bwd(ops._ptr(qkv), ops._ptr(o), ops._ptr(do), ops._ptr(L), ops._dt(qkv), B, S, H, D, rot, ops._ptr(tabs[0]),
                                             ops._ptr(tabs[1]), ops._ptr(am), case.T, ops._ptr(third), ops._ptr(delta), ops._stream()), "mafed_attn_bwd")
    torch.cuda.synchronize()
    assert plain.dtype == dt
    assert torch.equal(plain, summed), f"{case.id}: dqkv differs with and without colsum"
    assert torch.equal(plain, third), f"{case.id}: a second backward gives other bits"
    return plain.cpu().view(B, S, H, 3, D).double(), delta.cpu().double(), col.cpu().double()


class _Worst:
    def __init__(self):
        self.w = {}

    def add(self, name, got, ref, bnd, where):
        assert got.shape == ref.shape == bnd.shape, (name, got.shape, ref.shape, bnd.shape)
        assert bool(torch.isfinite(got).all()), f"{name}: non-finite at {where}"
        ratio = (got - ref).abs() / bnd
        x = float(ratio.max())
        if x >= self.w.get(name, (-1.0, None))[0]:
            self.w[name] = (x, (where, [int(i) for i in (ratio == ratio.max()).nonzero()[0]]))

    def __str__(self):
        return ", ".join(f"{k} {x:.3f}" for k, (x, _) in self.w.items())


def _check_backward(case, inp, ops, tabs, out, lse, worst, tag, where):
    dt = A.DTYPES[case.dtype]
    B, S, H, D = case.B, case.S, case.H, case.D
    r = T.backward(inp["qkv"], out, inp["dout"], lse, inp["vis"], inp["cos"], inp["sin"])
    bnd = T.backward_bound(inp["qkv"], out, inp["dout"], lse, inp["vis"], inp["cos"], inp["sin"], r, case.path, dt)
    c0 = 0.5 + (torch.arange(3 * H * D, dtype=torch.float32) % 7) * 0.25
    dqkv, delta, col = _backward(case, inp, ops, tabs, out, lse, c0)
    for i, name in enumerate(("dq", "dk", "dv")):
        worst.add(tag + name, dqkv[:, :, :, i], r[name], bnd[name], where)
    worst.add(tag + "delta", delta, r["delta"], bnd["delta"], where)
    worst.add(tag + "colsum", col, c0.double() + r["colsum"], bnd["colsum"] + B * S * T.U24 * c0.double(), where)
    pad = inp["pad"]
    assert bool((dqkv[:, :, :, 1:][pad] == 0).all()), f"{case.id} {where}: a padded key received gradient"


@pytest.mark.parametrize("case,fam", CASES, ids=[f"{c.id}-{f}" for c, f in CASES])
def test_kernels_are_within_the_bounds_of_the_fp64_reference(case, fam):
    from mafed_amd import ops
    dt = A.DTYPES[case.dtype]
    B, S, H, D = case.B, case.S, case.H, case.D
    worst = _Worst()
    for hot in T.variants(case, fam):
        inp = T.build(case, fam, hot)
        tabs = [t.to(DEV) for t in T.kernel_tables(inp["cos"], inp["sin"])]
        f = T.forward(inp["qkv"], inp["causal"], inp["pad"], inp["cos"], inp["sin"])
        out_k, lse_k = _forward(case, inp, ops, tabs)
        worst.add("out", out_k.double(), f["out"], T.out_bound(f, case.path, dt), hot)
        worst.add("lse", lse_k.double(), f["lse"], T.lse_bound(f, case.path), hot)
        if case.backward:
            out, lse = T.handed_over(case, f)
            _check_backward(case, inp, ops, tabs, out, lse, worst, "", hot)
            _check_backward(case, inp, ops, tabs, out_k.double().view(B, S, H, D), lse_k.double(), worst, "coupled ", hot)
    print(f"[attn-train] {case.label} | {fam} | {case.id} | worst err / bound: {worst}")
    bad = {k: v for k, v in worst.w.items() if not v[0] <= 1.0}
    assert not bad, f"{case.id} {fam} ({case.label}): err / bound = {worst}; beyond the bound at (hot row, index): {bad}"
