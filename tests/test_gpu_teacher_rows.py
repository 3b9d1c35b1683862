"""GPU: the distillation kernels reading teacher rows where they are stored -- through a per-sample index into a cache slab
[n, S, h], in fp32 or bf16 (``ops.TeacherRows``) -- instead of from a dense fp32 [B, S, h] copy of the batch's rows.

  * fp32 + index must give the BITS of today's call on the gathered tensor (the same kernel instantiation on the same values).
  * a bf16 teacher, with and without an index, is held to the fp64 restatements of tests/helpers.py evaluated on the rounded teacher
    ``t.bfloat16().double()``, at the bounds the existing tests hold the fp32 teacher to (KERNEL_RTOL, LN_INJECT_RTOL, the 1e-5 of
    test_distill's CLS check, the 1e-5 of test_layernorm_bwd_step_configuration's dx / dxsum): the rounded rows are exact fp32
    values, so nothing about the arithmetic after the load differs.
  * the argument checks of the new entry points.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import vlpythia_ref as R
from tests.helpers import KERNEL_RTOL, LN_INJECT_RTOL, assert_rel_close, distill_rows_fp64, ln_injection_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"
HS = [128, 768, 1024, 2048]
SMALL = dict(B=3, P=8, T=6, n=7, index=(6, 0, 3))      # 42 rows: not a multiple of the four rows of a block
MANY = dict(B=16, P=256, T=32, n=19, index=(18, 0, 3, 7, 13, 11, 2, 17, 5, 1, 16, 9, 4, 12, 8, 14))   # 4608 rows > 4 x DS_MAX_BLOCKS


def _ops():
    from mafed_amd import ops
    return ops


def D(v):
    return v.to(DEV)


def assert_close(a, b, tol, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= tol * max(1.0, float(b.abs().max())), f"{what}: max err {err:.3e}"


def _mask(B, T, g):
    """Left padding of random length; sample 0 keeps all of its text."""
    am = torch.ones(B, T, dtype=torch.int64)
    for b in range(1, B):
        am[b, : int(torch.randint(0, T, (1,), generator=g))] = 0
    return am


@functools.lru_cache(maxsize=None)
def _distill_case(h, shape, noise=0.3):
    """Student [B, S, h], mask, a cache slab [n, S, h] whose indexed samples are student + noise, and per loss the fp64 sums / ds
    on the bf16-rounded teacher.  Built once per shape; nothing in it is written afterwards."""
    sp = MANY if shape == "many" else SMALL
    B, P, T, n = sp["B"], sp["P"], sp["T"], sp["n"]
    S = P + T
    g = torch.Generator().manual_seed(1000 + h + B)
    index = torch.tensor(sp["index"], dtype=torch.int32)
    s = torch.randn(B, S, h, generator=g)
    slab = torch.randn(n, S, h, generator=g)
    slab[index.long()] = s + noise * torch.randn(B, S, h, generator=g)
    am = _mask(B, T, g)
    lang, img = R.modality_masks(am, P)
    coef = torch.tensor([0.3 / float(lang.sum()), 1.1 / float(img.sum())])
    t16 = slab.bfloat16()[index.long()]                 # the rounded rows of the batch
    ref = {cos: distill_rows_fp64(s, t16.double(), am, P, coef, cos) for cos in (False, True)}
    sd = s.double().requires_grad_(True)
    cls = R.cls_cos(sd, t16.double())
    cls.backward()
    return dict(B=B, P=P, T=T, S=S, h=h, n=n, s=s, slab=slab, index=index, am=am, coef=coef, t16=t16, ref=ref,
                counts=(float(lang.sum()), float(img.sum())), cls=cls.detach(), cls_grad=sd.grad)


# ---------------------------------------------------------------------------------------------------------------
# distill_fwd / distill_bwd / CLS
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("h,shape", [(h, "small") for h in HS] + [(128, "many")])
def test_fp32_index_gives_the_bits_of_the_gathered_tensor(h, shape, cosine):
    ops = _ops()
    c = _distill_case(h, shape)
    s, slab, index, am, coef, P = D(c["s"]), D(c["slab"]), D(c["index"]), D(c["am"]), D(c["coef"]), c["P"]
    gathered = slab[index.long()].contiguous()
    rows = ops.TeacherRows(slab, index)
    assert torch.equal(rows.materialize(), gathered)
    assert torch.equal(ops.distill_fwd(s, rows, am, P, cosine), ops.distill_fwd(s, gathered, am, P, cosine))
    assert torch.equal(ops.distill_bwd(s, rows, am, P, coef, cosine), ops.distill_bwd(s, gathered, am, P, coef, cosine))
    base = torch.randn(s.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    a, b = base.clone(), base.clone()
    ops.distill_bwd(s, rows, am, P, coef, cosine, out=a, accumulate=True)
    ops.distill_bwd(s, gathered, am, P, coef, cosine, out=b, accumulate=True)
    assert torch.equal(a, b)
    if cosine:
        cc = torch.tensor([1.0 / c["B"]], device=DEV)
        assert torch.equal(ops.distill_cls_fwd(s, rows), ops.distill_cls_fwd(s, gathered))
        assert torch.equal(ops.distill_cls_bwd(s, rows, cc), ops.distill_cls_bwd(s, gathered, cc))


@pytest.mark.parametrize("indexed", [True, False])
@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("h,shape", [(h, "small") for h in HS] + [(128, "many")])
def test_bf16_teacher_against_fp64_on_the_rounded_rows(h, shape, cosine, indexed):
    ops = _ops()
    c = _distill_case(h, shape)
    s, am, coef, P, B = D(c["s"]), D(c["am"]), D(c["coef"]), c["P"], c["B"]
    slab16 = D(c["slab"]).bfloat16()
    assert torch.equal(slab16.cpu()[c["index"].long()], c["t16"])
    rows = ops.TeacherRows(slab16, D(c["index"])) if indexed else ops.TeacherRows(D(c["t16"]))
    ref_sums, ref_ds = c["ref"][cosine]
    out = ops.distill_fwd(s, rows, am, P, cosine).cpu()
    assert (float(out[2]), float(out[3])) == c["counts"]
    assert_rel_close(out[0], ref_sums[0], KERNEL_RTOL, "lang sum")
    assert_rel_close(out[1], ref_sums[1], KERNEL_RTOL, "vision sum")
    ds = ops.distill_bwd(s, rows, am, P, coef, cosine)
    assert_rel_close(ds, ref_ds, KERNEL_RTOL, "ds")
    base = torch.ones_like(s)
    ops.distill_bwd(s, rows, am, P, coef, cosine, out=base, accumulate=True)
    assert_rel_close(base, ref_ds + 1.0, KERNEL_RTOL, "ds accumulate")
    if cosine:
        assert_close(ops.distill_cls_fwd(s, rows).reshape(()), c["cls"], 1e-5, "cls")
        assert_close(ops.distill_cls_bwd(s, rows, torch.tensor([1.0 / B], device=DEV)), c["cls_grad"], 1e-5, "cls grad")


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm backward with the injection
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_case(h, B, P, T, n, lp):
    """Inputs of the LayerNorm backward as the step runs it (both LayerNorms, residual gradient, DXSUM), a cache slab whose indexed
    samples are x + noise.  ``lp``: bf16 dY and the bf16 copy of dx (the bf16 step); else fp32 dY (the fp32 step)."""
    S = P + T
    rows = B * S
    g = torch.Generator().manual_seed(7 * h + B)
    index = torch.tensor(SMALL["index"], dtype=torch.int32) if B == 3 else torch.randperm(n, generator=g)[:B].to(torch.int32)
    if B != 3:
        index[0] = n - 1
    x = torch.randn(rows, h, generator=g) * 1.5 + 0.2
    slab = torch.randn(n, S, h, generator=g)
    slab[index.long()] = (x + 0.05 * torch.randn(rows, h, generator=g)).view(B, S, h)
    w1, w2 = 1 + 0.1 * torch.randn(h, generator=g), 1 + 0.1 * torch.randn(h, generator=g)
    b1, b2 = 0.1 * torch.randn(h, generator=g), 0.1 * torch.randn(h, generator=g)
    dy1, dy2 = 0.02 * torch.randn(rows, h, generator=g), 0.02 * torch.randn(rows, h, generator=g)
    if lp:
        dy1, dy2 = dy1.bfloat16(), dy2.bfloat16()
    dres = 0.02 * torch.randn(rows, h, generator=g)
    am = _mask(B, T, g)
    return dict(B=B, P=P, T=T, S=S, h=h, rows=rows, n=n, index=index, x=x, slab=slab, w=(w1, b1, w2, b2), dy=(dy1, dy2), dres=dres, am=am, lp=lp)


def _scales(h, cosine):
    # injection a few 1e-3 of dx, as in test_layernorm_bwd_step_configuration
    return torch.tensor([0.7, 0.4]) * (0.3 * math.sqrt(h) if cosine else 2e-3 * h), (-1.0 if cosine else 2.0 / h)


def _ln_run(ops, c, teacher, scales, inj_mul, split):
    """-> (dx, dx_lp, [dw1, db1, dw2, db2, dxsum_a, dxsum_b]) of one form of the backward; teacher None = no injection"""
    x, (w1, b1, w2, b2), (dy1, dy2) = D(c["x"]), [D(v) for v in c["w"]], [D(v) for v in c["dy"]]
    _, _, mean, rstd = ops.layernorm_fwd(x, w1, b1, w2, b2, 1e-5, torch.float32)
    kw = dict(teacher=teacher, attention_mask=D(c["am"]), S=c["S"], P=c["P"], inj_scale=D(scales), inj_mul=inj_mul) if teacher is not None else {}
    grads = [torch.zeros(c["h"], device=DEV) for _ in range(6)]
    if split:
        dx, dx_lp, ws = ops.layernorm_bwd_rows(dy1, dy2, x, mean, rstd, w1, w2, D(c["dres"]), want_lp=c["lp"], want_dxsum=True, **kw)
        ops.layernorm_bwd_params(ws, c["rows"], c["h"], *grads)
    else:
        dx, dx_lp = ops.layernorm_bwd(dy1, dy2, x, mean, rstd, w1, w2, D(c["dres"]), *grads[:4], want_lp=c["lp"], dxsum_a=grads[4],
                                      dxsum_b=grads[5], **kw)
    return dx, dx_lp, grads


LN_SHAPES = [(h, 3, 8, 6, 7, h >= 1024) for h in HS] + [(1024, 32, 256, 32, 33, True)]     # the last: 9216 x 1024, the step's own


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("h,B,P,T,n,lp", LN_SHAPES)
def test_layernorm_injection_fp32_index_gives_the_bits_of_the_gathered_tensor(h, B, P, T, n, lp, cosine):
    ops = _ops()
    c = _ln_case(h, B, P, T, n, lp)
    scales, inj_mul = _scales(h, cosine)
    slab, index = D(c["slab"]), D(c["index"])
    gathered = slab[index.long()].contiguous().view(c["rows"], h)
    for split in (False, True):
        a = _ln_run(ops, c, ops.TeacherRows(slab, index), scales, inj_mul, split)
        b = _ln_run(ops, c, gathered, scales, inj_mul, split)
        assert torch.equal(a[0], b[0]), "dx"
        assert (a[1] is None and b[1] is None) if not lp else torch.equal(a[1], b[1]), "dx_lp"
        for u, v, what in zip(a[2], b[2], ("dw1", "db1", "dw2", "db2", "dxsum_a", "dxsum_b")):
            assert torch.equal(u, v), what


@pytest.mark.parametrize("indexed", [True, False])
@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("h,B,P,T,n,lp", LN_SHAPES)
def test_layernorm_injection_bf16_teacher_against_fp64(h, B, P, T, n, lp, cosine, indexed):
    ops = _ops()
    c = _ln_case(h, B, P, T, n, lp)
    scales, inj_mul = _scales(h, cosine)
    rows, S = c["rows"], c["S"]
    slab16 = D(c["slab"]).bfloat16()
    t16 = slab16[D(c["index"]).long()].contiguous()
    teacher = ops.TeacherRows(slab16, D(c["index"])) if indexed else ops.TeacherRows(t16)
    inj = ln_injection_fp64(c["x"], t16.cpu().view(rows, h), c["am"], S, c["P"], scales, inj_mul)
    small = B == 3
    if small:
        xd = c["x"].double().requires_grad_(True)
        w1, b1, w2, b2 = (v.double() for v in c["w"])
        dy1, dy2 = (v.double() for v in c["dy"])
        ((F.layer_norm(xd, (h,), w1, b1, 1e-5) * dy1).sum() + (F.layer_norm(xd, (h,), w2, b2, 1e-5) * dy2).sum() + (xd * c["dres"].double()).sum()).backward()
        ref_dx = xd.grad + inj
    for split in (False, True):
        dx, dx_lp, grads = _ln_run(ops, c, teacher, scales, inj_mul, split)
        dx0, _, _ = _ln_run(ops, c, None, scales, inj_mul, split)
        assert_rel_close(dx.cpu() - dx0.cpu(), inj, LN_INJECT_RTOL, "injection dx(with) - dx(without)")
        if lp:
            assert torch.equal(dx_lp, dx.to(torch.bfloat16))
        if small:
            assert_rel_close(dx, ref_dx, 1e-5, "dx")
            assert_rel_close(grads[4], ref_dx.sum(0), 1e-5, "dxsum_a")
            assert_rel_close(grads[5], ref_dx.sum(0), 1e-5, "dxsum_b")


# ---------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from mafed_amd import _lib
    ops = _ops()
    B, P, T, n = 3, 8, 6, 7
    S = P + T
    am = torch.ones(B, T, dtype=torch.int64, device=DEV)
    index = torch.tensor([6, 0, 3], dtype=torch.int32, device=DEV)
    coef = torch.tensor([0.5, 0.5], device=DEV)

    def every_distill_op(s, rows):
        for call in (lambda: ops.distill_fwd(s, rows, am, P), lambda: ops.distill_bwd(s, rows, am, P, coef),
                     lambda: ops.distill_cls_fwd(s, rows), lambda: ops.distill_cls_bwd(s, rows, coef[:1])):
            with pytest.raises(_lib.MafedHipError, match="rc=-1"):
                call()

    # a bf16 base that is not 8-byte aligned
    h = 128
    s = torch.zeros(B, S, h, device=DEV)
    buf = torch.zeros(n * S * h + 4, dtype=torch.bfloat16, device=DEV)
    odd = ops.TeacherRows(buf[1: 1 + n * S * h].view(n, S, h), index)
    assert odd.states.data_ptr() % 8 == 2
    every_distill_op(s, odd)
    x = torch.zeros(B * S, h, device=DEV)
    w = torch.ones(h, device=DEV)
    _, _, mean, rstd = ops.layernorm_fwd(x, w, w, None, None, 1e-5, torch.float32)
    g1, g2 = torch.zeros(h, device=DEV), torch.zeros(h, device=DEV)
    inj = dict(attention_mask=am, S=S, P=P, inj_scale=coef, inj_mul=2.0 / h)
    with pytest.raises(_lib.MafedHipError, match="rc=-1"):
        ops.layernorm_bwd(x, None, x, mean, rstd, w, None, None, g1, g2, teacher=odd, **inj)
    with pytest.raises(_lib.MafedHipError, match="rc=-1"):
        ops.layernorm_bwd_rows(x, None, x, mean, rstd, w, None, None, teacher=odd, **inj)
    # h % 4 != 0
    h6 = 6
    every_distill_op(torch.zeros(B, S, h6, device=DEV), ops.TeacherRows(torch.zeros(n, S, h6, dtype=torch.bfloat16, device=DEV), index))
    # an index without the teacher it indexes
    lib = _lib.load()
    ws = torch.empty(lib.mafed_layernorm_bwd_workspace_bytes(B * S, h), dtype=torch.uint8, device=DEV)
    dx = torch.empty_like(x)
    p = lambda t: t.data_ptr()
    with pytest.raises(_lib.MafedHipError, match="rc=-1"):
        ops.check(lib.mafed_layernorm_bwd_indexed(p(x), 0, _lib.F32, p(x), p(mean), p(rstd), p(w), 0, B * S, h, 0, p(dx), 0, p(g1), p(g2), 0, 0,
                                                  0, _lib.F32, p(index), p(am), S, P, T, p(coef), 2.0 / h, 0, 0, p(ws), ws.numel(), 0),
                  "mafed_layernorm_bwd_indexed")
    with pytest.raises(_lib.MafedHipError, match="rc=-1"):
        ops.check(lib.mafed_layernorm_bwd_rows_indexed(p(x), 0, _lib.F32, p(x), p(mean), p(rstd), p(w), 0, B * S, h, 0, p(dx), 0, 0, _lib.F32,
                                                       p(index), p(am), S, P, T, p(coef), 2.0 / h, 0, p(ws), ws.numel(), 0),
                  "mafed_layernorm_bwd_rows_indexed")
    torch.cuda.synchronize()
