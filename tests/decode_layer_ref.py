"""fp64 reference of the fused decode-layer kernels (mafed_amd/csrc/decode.hip), stated at the kernels' interface, with the per-element
error bound their outputs are held to, the inputs that make a wrong fragment / parameter / slice visible, and the case list with the
dispatch arithmetic that says which kernel a case reaches.  Plain torch, CPU; nothing here imports ``mafed_amd``.

Three entry points:

    ln_qkv_fc1   qkv = LN1(x) wqkv^T + bqkv                     a = gelu(LN2(x) w1^T + bfc1)          (bf16 out)
    ln_linear    logits = LN(x) w^T (+ bias)                                                           (bf16 out)
    out          x' = x + bd + b2 + ao wd^T + act w2^T                                                 (fp32 out)

LayerNorm is the biased-variance form with eps inside the root, GELU the exact erf form.

The error model (per output element n of row m; u = 2^-24, line numbers of decode.hip):

  * Operand rounding.  The kernels round the normalised row to bf16 before the MFMA (:148, the store4 of :321 / :460).  The reference
    does the same: y in fp64, yb = bf16(y), product from yb in fp64.  That rounding is then part of the reference, not of the bound.
  * Uncertain elements.  The kernel's y comes from fp32 arithmetic and may land on the other side of a bf16 rounding boundary.  With
    |y32 - y| <= delta (below) and rounding monotone, bf16(y - delta) <= bf16(y32) <= bf16(y + delta): where the two ends agree the
    kernel's operand IS yb; elsewhere it is off by at most unc = bf16(y + delta) - bf16(y - delta) (one bf16 ulp).  Output n gains
    sum_k |w_nk| unc_k.
  * delta: first-order error of the two-pass fp32 LayerNorm (``ln_delta``).
      - mean: a sum of h terms in a tree of depth S_MEAN = 13 + h / 256 (direct form :106-117: 3 levels inside a fragment, KS = h / 256
        fragments in turn, 2 shuffles, 8 waves in turn; the LDS forms :290-299, :431-440 are shallower: 2 + 4 + 6 = 12 at h = 1024)
        and one division:  |dmu| <= (S_MEAN + 1) u mean|x|.
      - second moment: d_k = fl(x_k - mean32) = (x_k - mu - dmu)(1 + e).  sum_k (x_k - mu - dmu)^2 = h var + h dmu^2 exactly (the cross
        term vanishes), so dmu enters at second order, (dmu / sigma)^2; the roundings of d (2 u), of the square (u) and of the sum
        (depth S_Q = h / 32 + 10: the direct form's fmaf chain over 8 KS elements :120-125, 2 shuffles, 8 waves) are relative errors of
        q; /h, + eps: u each; root and reciprocal (:136): one ulp = 2 u each.
            r = (S_Q + 5) u / 2 + 4 u + (dmu / sigma)^2 / 2           relative error of rstd
      - z32 = fl(d32 rstd32):  |z32 - z| <= |z| (r + 2 u) + |dmu| / sigma
      - y32 = fl(fl(z32 g) + b):  delta = |g| |z32 - z| + u |g z| + u |y|
    delta grows with |x|max / sigma of the row through dmu / sigma.
  * fp32 accumulation.  C_ACC (K / 32 + 8 + P) u A_n with A_n = sum_k |w_nk yb_k|: K / 32 MFMA steps, the 8-wave (:168, :360, :496) or
    4-lane (:576) fold through LDS, P slices (:550).  C_ACC = 8: an MFMA 16x16x32 folds 32 products into the accumulator; neither the
    association nor the rounding mode of its internal adds is documented, so each of the 4 eight-element fragments of an instruction
    is allowed one rounding of a full ulp (2 u, truncation).  The LDS fold and the slice sum are plain fp32 adds (u each) and lie
    under the same constant.
  * bias add (:171, :363): u |ref|.
  * qkv and logits: half a bf16 ulp of the stored value (store4 -> f32_to_bf16).
  * fc1: the pre-activation bound times the Lipschitz constant of GELU (max gelu' = 1.129 < 1.13), 5e-5 for the polynomial
    (gelu_erf_fast, common.h: the bound tests/test_gpu_kernels.py::test_fast_gelu_polynomials_against_erf holds it to on [-8, 8]; a case
    whose pre-activations leave [-8, 8] is rejected), half a bf16 ulp.
  * decode_out: operands are bf16 already.  Accumulation as above with K = h + n1 and P = 16 (the largest P the dispatch forms);
    the epilogue r + (v + c0 + c1) (:600): two roundings of sums bounded by A_n + |bd| + |b2|, and half an fp32 ulp of x'.
  * Cap.  A case whose uncertain share exceeds 1 % of the operand elements is rejected (``normalised`` asserts).

Input families (``a_inputs`` / ``out_inputs``): distinct, edge (offset + smallvar rows), census; random, integers.
tests/test_decode_layer_ref.py shows on the CPU that the bound on these inputs sees the mistakes it is there for."""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import torch

F64 = torch.float64
U24 = 2.0 ** -24
C_ACC = 8.0
P_MAX = 16
GELU_LIP = 1.13
GELU_POLY = 5e-5
GELU_RANGE = 8.0
UNCERTAIN_CAP = 0.01
EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------------------
# number formats
# ------------------------------------------------------------------------------------------------------------------------------
def _exponent(v: torch.Tensor) -> torch.Tensor:
    """e with |v| = mant * 2^e, mant in [0.5, 1); the smallest normal fp32 / bf16 exponent for 0 and below"""
    _, e = torch.frexp(v.double().abs())
    return torch.where(v == 0, torch.full_like(e, -125), e).clamp(min=-125)


def bf16_round(v: torch.Tensor) -> torch.Tensor:
    """fp64 -> nearest bf16 (8 significant bits, ties to even), as fp64; one rounding, not two through fp32"""
    e = _exponent(v)
    scale = torch.ldexp(torch.ones_like(v, dtype=F64), 8 - e)
    return torch.round(v.double() * scale) / scale


def half_ulp(v: torch.Tensor, bits: int) -> torch.Tensor:
    """half an ulp of a format with ``bits`` significant bits at |v|"""
    return torch.ldexp(torch.ones_like(v, dtype=F64), _exponent(v) - bits - 1)


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
def row_stats(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    x = x.double()
    mu = x.mean(dim=-1, keepdim=True)
    return mu, ((x - mu) ** 2).mean(dim=-1, keepdim=True)


def layer_norm(x, g, b, eps: float) -> torch.Tensor:
    mu, var = row_stats(x)
    return (x.double() - mu) / torch.sqrt(var + eps) * g.double() + b.double()


def gelu(u: torch.Tensor) -> torch.Tensor:
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def ln_delta(x, g, b, eps: float) -> torch.Tensor:
    """|y32 - y| of the two-pass fp32 LayerNorm, first order (derivation: module docstring)"""
    h = x.shape[-1]
    x, g, b = x.double(), g.double(), b.double()
    mu, var = row_stats(x)
    sig = torch.sqrt(var + eps)
    z = (x - mu) / sig
    y = z * g + b
    dmu = (13 + h / 256 + 1) * U24 * x.abs().mean(dim=-1, keepdim=True)
    s_q = h / 32 + 10
    r = 0.5 * (s_q + 5) * U24 + 4 * U24 + 0.5 * (dmu / sig) ** 2
    dz = z.abs() * (r + 2 * U24) + dmu / sig
    return g.abs() * dz + U24 * (g * z).abs() + U24 * y.abs()


@dataclass
class Operand:
    """The bf16 MFMA operand of a LayerNorm prologue: y fp64, yb = bf16(y), unc = how far the kernel's operand may lie from yb"""
    y: torch.Tensor
    yb: torch.Tensor
    unc: torch.Tensor

    @property
    def share(self) -> float:
        return float((self.unc > 0).double().mean())


def normalised(x, g, b, eps: float, cap: Optional[float] = UNCERTAIN_CAP) -> Operand:
    y = layer_norm(x, g, b, eps)
    d = ln_delta(x, g, b, eps)
    op = Operand(y=y, yb=bf16_round(y), unc=bf16_round(y + d) - bf16_round(y - d))
    assert bool((op.unc >= 0).all())
    if cap is not None:
        assert op.share <= cap, f"uncertain share {op.share:.4f} above the cap {cap}: the input is too harsh for this bound"
    return op


def _linear(op: Operand, w, bias) -> Dict[str, torch.Tensor]:
    """ref = yb w^T + bias with what the bound needs: pre = everything in front of the last rounding"""
    w = w.double()
    K = w.shape[1]
    ref = op.yb @ w.t()
    A = op.yb.abs() @ w.abs().t()
    if bias is not None:
        ref = ref + bias.double()
        A = A + bias.double().abs()
    pre = op.unc @ w.abs().t() + C_ACC * (K / 32 + 8) * U24 * A + U24 * ref.abs()
    return {"ref": ref, "A": A, "pre": pre}


def _bf16_store(lin: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {"ref": lin["ref"], "bound": lin["pre"] + half_ulp(lin["ref"].abs() + lin["pre"], 8)}


def _gelu_store(lin: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    assert float((lin["ref"].abs() + lin["pre"]).max()) <= GELU_RANGE, "a pre-activation outside the range the polynomial is bounded on"
    ref = gelu(lin["ref"])
    pre = GELU_LIP * lin["pre"] + GELU_POLY
    return {"ref": ref, "bound": pre + half_ulp(ref.abs() + pre, 8)}


def ln_qkv_fc1(x, g1, b1, g2, b2, eps, wqkv, bqkv, w1, bfc1, cap: Optional[float] = UNCERTAIN_CAP):
    """-> (qkv, a): each {"ref", "bound"} [M, N], and the two operands"""
    o1, o2 = normalised(x, g1, b1, eps, cap), normalised(x, g2, b2, eps, cap)
    qkv, a = _bf16_store(_linear(o1, wqkv, bqkv)), _gelu_store(_linear(o2, w1, bfc1))
    qkv["op"], a["op"] = o1, o2
    return qkv, a


def ln_linear(x, g, b, eps, w, bias=None, cap: Optional[float] = UNCERTAIN_CAP):
    o = normalised(x, g, b, eps, cap)
    res = _bf16_store(_linear(o, w, bias))
    res["op"] = o
    return res


def out(x, ao, act, wd, bd, w2, b2):
    """-> {"ref", "bound"} [M, h] of x' = x + bd + b2 + ao wd^T + act w2^T"""
    x, ao, act, wd, bd, w2, b2 = (t.double() for t in (x, ao, act, wd, bd, w2, b2))
    h, n1 = wd.shape[0], w2.shape[1]
    prod = ao @ wd.t() + act @ w2.t()
    A = ao.abs() @ wd.abs().t() + act.abs() @ w2.abs().t()
    ref = x + bd + b2 + prod
    rest = C_ACC * ((h + n1) / 32 + 8 + P_MAX) * U24 * A + 2 * U24 * (A + bd.abs() + b2.abs())
    return {"ref": ref, "bound": rest + half_ulp(ref.abs() + rest, 24), "A": A}


# ------------------------------------------------------------------------------------------------------------------------------
# census: W[n, :] = e_k(n)
# ------------------------------------------------------------------------------------------------------------------------------
def census_k(N: int, h: int) -> torch.Tensor:
    """k(n) = (7 n + 3) mod h: a bijection on every run of h columns (7 is prime to h = 256 KS), so N >= h columns read every k"""
    return (7 * torch.arange(N) + 3) % h


def census_weight(N: int, h: int) -> torch.Tensor:
    w = torch.zeros(N, h, dtype=torch.bfloat16)
    w[torch.arange(N), census_k(N, h)] = 1.0
    return w


def census_check(got: torch.Tensor, op: Operand, N: int) -> Tuple[int, float]:
    """got [M, N] (bf16 values) of a census product without bias -> (elements outside the uncertain set that are not bf16(y[m, k(n)])
    bit for bit, worst |got - yb| / unc inside the set)"""
    k = census_k(N, op.y.shape[1])
    yb, unc = op.yb[:, k], op.unc[:, k]
    err = (got.double() - yb).abs()
    sure = unc == 0
    wrong = int(((err != 0) & sure).sum())
    inside = float((err[~sure] / unc[~sure]).max()) if bool((~sure).any()) else 0.0
    return wrong, inside


# ------------------------------------------------------------------------------------------------------------------------------
# dispatch, restated (decode.hip: decode_a_launch, mafed_decode_ln_qkv_fc1, mafed_decode_ln_linear, mafed_decode_out)
# ------------------------------------------------------------------------------------------------------------------------------
def a_form(M: int, h: int, lds: bool) -> Tuple[str, int, int]:
    """-> (form, MT, KS)"""
    mt, ks = (M + 15) // 16, h // 256
    if lds and mt <= 2 and ks == 4 and (16 * mt + 32) * (h + 8) * 2 <= 160 * 1024:
        return "lds", mt, ks
    return "direct", mt, ks


def late_gb(mt: int, ks: int, np_: int = 1) -> bool:
    return ks == 8 or mt * ks >= 16 or np_ > 1


def linear_path(M: int, h: int, N: int, bias: bool, cus: int, lds: bool = True) -> str:
    mt, ks = (M + 15) // 16, h // 256
    if lds and mt <= 2 and ks == 4 and not bias and N % 16 == 0 and N // 16 >= 4 * cus:
        return "head"
    if lds and mt <= 2 and ks == 4 and (16 * mt + 32) * (h + 8) * 2 <= 160 * 1024:
        return "lds"
    if N % 128 == 0 and mt <= 2 and ks <= 4 and N // 128 >= 2 * cus:
        return "np4"
    return "np1"


def out_plan(M: int, h: int, n1: int, cus: int, lds: bool) -> Tuple[str, int, int]:
    """-> (form, P, k-steps per slice)"""
    mt, groups, ktot = (M + 15) // 16, h // 32, (h + n1) // 32
    P = min(16, max(1, (cus + groups // 2) // groups))
    ksl = (-(-ktot // P) + 3) // 4 * 4
    P = -(-ktot // ksl)
    if lds and mt <= 2 and h == 1024 and n1 % 512 == 0 and -(-ktot // 16) <= 16:
        return "lds", -(-ktot // 16), 16
    return "direct", P, ksl


def straddles(h: int, P: int, ksl: int) -> bool:
    """a slice holds k-steps of both the dense and the fc2 operand"""
    kh = h // 32
    return kh % ksl != 0 and kh // ksl < P


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
CUS = 256   # the CU count the shapes below were chosen for; the GPU test asserts on the device's own count where each case lands


@dataclass(frozen=True)
class ACase:
    M: int
    h: int
    n1: int = 32
    lds: bool = False     # variant 761 (True) or 760
    form: str = "direct"  # where it must land

    @property
    def id(self) -> str:
        return f"A-M{self.M}h{self.h}n{self.n1}-{'v761' if self.lds else 'v760'}-{self.form}"


@dataclass(frozen=True)
class LCase:
    M: int
    h: int
    N: int
    bias: bool
    path: str             # head | lds | np4 | np1
    families: Tuple[str, ...] = ("distinct", "edge")

    @property
    def id(self) -> str:
        return f"L-M{self.M}h{self.h}N{self.N}{'b' if self.bias else ''}-{self.path}"


@dataclass(frozen=True)
class OCase:
    M: int
    h: int
    n1: int
    lds: bool
    form: str
    P: int                # at CUS compute units
    note: str = ""

    @property
    def id(self) -> str:
        return f"O-M{self.M}h{self.h}n{self.n1}-{'v761' if self.lds else 'v760'}-{self.form}P{self.P}"


def a_cases() -> List[ACase]:
    c: List[ACase] = []
    for ks in (1, 2, 3, 4):
        c += [ACase(M=16 * mt - 3, h=256 * ks) for mt in (1, 2, 3, 4)]
    c += [ACase(M=16 * mt - 3, h=2048) for mt in (1, 2)]
    c += [ACase(M=16 * mt, h=256 * ks) for ks, mt in ((1, 4), (2, 3), (3, 2), (4, 1), (8, 2))]      # M = 16 MT exactly
    c += [ACase(M=M, h=1024, lds=True, form="lds") for M in (5, 16, 29, 32)]
    c.append(ACase(M=33, h=1024, lds=True, form="direct"))
    # fc1 as wide as h: the census reads every k through the second segment too
    c += [ACase(M=13, h=256, n1=256), ACase(M=29, h=1024, n1=1024, lds=True, form="lds")]
    return c


def l_cases() -> List[LCase]:
    c: List[LCase] = [LCase(M=13, h=1024, N=32, bias=True, path="lds"), LCase(M=29, h=1024, N=96, bias=True, path="lds")]
    for M in (3, 32):
        c.append(LCase(M=M, h=1024, N=64 * CUS, bias=False, path="head", families=("distinct", "edge", "census") if M == 32 else ("distinct", "edge")))
        c.append(LCase(M=M, h=1024, N=64 * CUS + 32, bias=False, path="head"))       # nstrips % grid != 0: unequal trip counts
    for h in (256, 768):
        for M in (7, 20):
            c.append(LCase(M=M, h=h, N=256 * CUS, bias=False, path="np4", families=("distinct", "edge", "census") if (h, M) == (768, 20) else ("distinct", "edge")))
    c.append(LCase(M=13, h=512, N=96, bias=False, path="np1"))
    c.append(LCase(M=13, h=2048, N=64, bias=True, path="np1"))
    return c


def out_cases() -> List[OCase]:
    c: List[OCase] = []
    for n1, P in ((32, 3), (1280, 12), (1408, 13), (1792, 16)):
        c += [OCase(M=16 * mt - 3, h=256, n1=n1, lds=False, form="direct", P=P) for mt in (1, 2, 3, 4)]
    c.append(OCase(M=13, h=768, n1=3712, lds=False, form="direct", P=9, note="slice 1 straddles k-step 24"))
    c.append(OCase(M=29, h=2048, n1=64, lds=False, form="direct", P=4, note="slice 3 straddles k-step 64"))
    for n1, P in ((512, 3), (7168, 16)):
        c += [OCase(M=M, h=1024, n1=n1, lds=True, form="lds", P=P) for M in (9, 32)]
    c.append(OCase(M=9, h=1024, n1=7680, lds=True, form="direct", P=8, note="17 LDS slices: falls back"))
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# inputs (every tensor holds values its kernel dtype represents exactly; the GPU test only casts)
# ------------------------------------------------------------------------------------------------------------------------------
A_FAMILIES = ("distinct", "edge", "census")
OUT_FAMILIES = ("random", "integers")


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def grid_weight(N: int, K: int, g: torch.Generator, gain: float = 1.0) -> torch.Tensor:
    """bf16 [N, K]: integers in -15 .. 15 times a power of two near gain / (8 sqrt K) (sigma about gain / sqrt K).  Exact in bf16,
    cheap to draw for a vocabulary-sized N."""
    scale = 2.0 ** round(math.log2(gain / (8.0 * math.sqrt(K))))
    return (torch.randint(-15, 16, (N, K), generator=g, dtype=torch.int8).to(torch.float32) * scale).to(torch.bfloat16)


def rows(fam: str, M: int, h: int, g: torch.Generator) -> torch.Tensor:
    """fp32 [M, h].  distinct / census: row m has mean 0.25 m - 2 and sigma 0.5 + m / 16 (|mean| / sigma <= 4: delta grows with it, and at 8
    the rows of h = 2048 exceed the 1 % cap).  edge: the same, but rows 0 and 17 are offset
    rows (mean 6, sigma 1; a mean of 8 puts that row near 2 % uncertain and a three-row case over the cap) and rows 1 and 16 smallvar rows
    (mean 0.02, sigma 0.01: eps = 1e-5 moves rstd by 5 %)."""
    m = torch.arange(M, dtype=torch.float32)[:, None]
    r = torch.randn(M, h, generator=g)
    x = r * (0.5 + m / 16) + (0.25 * m - 2)
    if fam == "edge":
        for row, (mean, sig) in ((0, (6.0, 1.0)), (1, (0.02, 0.01)), (16, (0.02, 0.01)), (17, (6.0, 1.0))):
            if row < M:
                x[row] = r[row] * sig + mean
    return x.contiguous()


def ln_params(h: int, g: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """gamma in [0.5, 2] (log-uniform), beta in [-1, 1]"""
    return (2.0 ** (torch.rand(h, generator=g) * 2 - 1)).float(), (torch.rand(h, generator=g) * 2 - 1).float()


def col_bias(N: int, g: torch.Generator) -> torch.Tensor:
    """O(1) and distinct per column: a ramp over four neighbours plus noise, so that a 4-column shift moves every element"""
    n = torch.arange(N)
    return (((n // 4) % 5 - 2).float() * 0.5 + 0.25 * torch.randn(N, generator=g)).float()


@lru_cache(maxsize=4)
def a_inputs(case: ACase, fam: str) -> Dict[str, torch.Tensor]:
    g = _gen(1, case.M, case.h, case.n1, A_FAMILIES.index(fam))
    h, n1 = case.h, case.n1
    x = rows(fam, case.M, h, g)
    g1, b1 = ln_params(h, g)
    g2, b2 = ln_params(h, g)
    if fam == "census":
        wqkv, w1 = census_weight(3 * h, h), census_weight(n1, h)
        bqkv, bfc1 = torch.zeros(3 * h), torch.zeros(n1)
    else:
        wqkv, w1 = grid_weight(3 * h, h, g), grid_weight(n1, h, g, gain=0.5)
        bqkv, bfc1 = col_bias(3 * h, g), col_bias(n1, g)
    return dict(x=x, g1=g1, b1=b1, g2=g2, b2=b2, wqkv=wqkv, bqkv=bqkv, w1=w1, bfc1=bfc1)


@lru_cache(maxsize=4)
def a_reference(case: ACase, fam: str):
    i = a_inputs(case, fam)
    return ln_qkv_fc1(i["x"], i["g1"], i["b1"], i["g2"], i["b2"], EPS, i["wqkv"], i["bqkv"], i["w1"], i["bfc1"])


@lru_cache(maxsize=2)
def l_inputs(case: LCase, fam: str) -> Dict[str, Optional[torch.Tensor]]:
    g = _gen(2, case.M, case.h, case.N, A_FAMILIES.index(fam))
    x = rows(fam, case.M, case.h, g)
    gm, bt = ln_params(case.h, g)
    if fam == "census":
        assert not case.bias
        w = census_weight(case.N, case.h)
    else:
        w = grid_weight(case.N, case.h, g)
    return dict(x=x, g=gm, b=bt, w=w, bias=col_bias(case.N, g) if case.bias else None)


@lru_cache(maxsize=2)
def l_reference(case: LCase, fam: str):
    i = l_inputs(case, fam)
    return ln_linear(i["x"], i["g"], i["b"], EPS, i["w"], i["bias"])


def out_operands(fam: str, M: int, h: int, n1: int) -> Dict[str, torch.Tensor]:
    g = _gen(3, M, h, n1, OUT_FAMILIES.index(fam))
    if fam == "integers":
        # asymmetric small integers: exact in bf16, and every partial sum (|.| <= 9 (h + n1) + 30 < 2^24) exact in fp32
        ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).float()
        return dict(x=ri(-8, 9, M, h), ao=ri(-2, 4, M, h).to(torch.bfloat16), act=ri(-2, 4, M, n1).to(torch.bfloat16),
                    wd=ri(-3, 3, h, h).to(torch.bfloat16), bd=ri(-5, 7, h), w2=ri(-3, 3, h, n1).to(torch.bfloat16), b2=ri(-6, 5, h))
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=(r(M, h) * 1.5 + 0.3).float(), ao=r(M, h).to(torch.bfloat16), act=(r(M, n1) + 0.25).to(torch.bfloat16),
                wd=grid_weight(h, h, g), bd=col_bias(h, g), w2=grid_weight(h, n1, g), b2=col_bias(h, g))


@lru_cache(maxsize=4)
def out_inputs(case: OCase, fam: str) -> Dict[str, torch.Tensor]:
    return out_operands(fam, case.M, case.h, case.n1)


@lru_cache(maxsize=4)
def out_reference(case: OCase, fam: str):
    i = out_inputs(case, fam)
    return out(i["x"], i["ao"], i["act"], i["wd"], i["bd"], i["w2"], i["b2"])
