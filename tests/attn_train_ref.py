"""fp64 reference of the training attention kernels (attn_mfma.hip: tiled and resident forward / dQ / dK dV; attn_ref.hip: the exact
row kernels), stated at the kernels' interface, with the per-element bounds their outputs are held to and the inputs that make one
wrong key, query, row statistic or rotation visible.  Plain torch, CPU; built on tests/attn_infer_ref.py (``Group``, ``attend``, the
forward bound and ``make_rows``); nothing here imports ``mafed_amd``.

Forward (``ops.attn_fwd``, ``ops.attn_fwd_exact_bf16``, ``ops.attn_fwd_bidir``): one ``Group`` per sample with all S queries, causal =
tril, pad from the left-padded mask (bidirectional: every key, no pad, no rotary).  ``out`` is held to ``attn_infer_ref.bound`` with
the path's terms; the resident kernel has an entry of its own (``RESIDENT``).  ``lse = m + log L`` (natural log, [B,H,S]) is held to

    bound_lse = 4 * rel + 4 u (|m| + |log L| + 2 lazy) + half an fp32 ulp of lse,    rel = 2 u_s sigma + u_exp(Delta) + u_p + (nk + D) u

  * rel is the relative error of every p_j of the row (attn_infer_ref), hence of the normaliser L, hence the absolute error of log L;
    d lse / d s_j = p_j, so the operand roundings of the scores enter through the same term;
  * the score at the maximum is formed in fp32 (s * scale, attn_mfma.hip:270; s * scale2, :868), carried as m and, in the resident
    kernel, multiplied by ln 2 (:925); logf(l) has an ulp of its own: 4 u (|m| + |log L|);
  * lazy = 8 ln 2 on the resident path: its running reference moves only when a row maximum outgrows it by 2^8 (:889), so the m and
    the l it adds can each be that much larger in magnitude than the true ones; 0 elsewhere.

Backward (``ops.attn_bwd``): a function of exactly what ``mafed_attn_bwd`` reads -- qkv, out, dout as the dtype holds them, lse in fp32,
the mask and the rotary tables.  Per (b, h), with q~, k~ the rotated rows,

    s_ij = <q~_i, k~_j> / sqrt D         p_ij = exp(s_ij - lse_i) on visible (i, j), else 0
    delta_i = sum_d dout_id out_id       dP_ij = <dout_i, v_j>                dS_ij = p_ij (dP_ij - delta_i)
    dV_j = sum_i p_ij dout_i             dK~_j = sum_i dS_ij q~_i / sqrt D    dQ~_i = sum_j dS_ij k~_j / sqrt D
    dq_i, dk_j = the transpose rotation at the row's own position; the plain dims pass through.

The backward's error model (first order, per output element; u = 2^-24; n_i / n_j = visible keys of row i / queries of key j):

    e_p(i,j)  = (2 u_s + D u) sabs_ij + exp_a + exp_b (|s_ij| + |lse_i|)
        relative error of p_ij.  sabs_ij = sum_d |q~|_id |k~|_jd / sqrt D, with |x~| = |x c| + |y s| the magnitude of the rotation's two
        products (a rotated element can be far smaller than they are, and is rounded at their size; the same |q~|, |k~| stand in
        E_K~ and E_Q~ below), scales the roundings of the rotated operands (u_s each) and
        the D-term fp32 chain under the score.  lse_i is an input, so the exponent's argument s_ij scale - lse_i is rounded at the
        magnitude of its two terms, not at their difference (attn_mfma.hip:551, :632, :1044-1050, :1185; attn_ref.hip:85, :144).
    e_d(i,j)  = D u (sum_d |dout_id v_jd| + sum_d |dout_id out_id|) + u |dP_ij - delta_i|
        absolute error of dP_ij - delta_i: two D-term fp32 chains and the subtraction.
    E_S(i,j)  = p_ij (e_p |dP_ij - delta_i| + e_d) + (u_p + 3 u) |dS_ij|
        absolute error of dS_ij as the second product reads it: the two fp32 products (p * (..) * scale) and, on the MFMA kernels, the
        bf16 rounding of dS (pack_acc, attn_mfma.hip:559, :639, :1054, :1197); u_p = 0 on the row kernels (sc / dsq stay fp32).
        (u_s, u_p here are BWD_PATHS': the bf16 unit roundoff 2^-8.  The forward keeps attn_infer_ref's 2^-9, the mean-case half ulp
        its bound was merged and measured with, so that both forward families are held to one formula; its factor 4 absorbs the
        difference, and the forward emulation stays at 0.33.  The backward's terms were derived here and use the worst case of the
        format; with 2^-9 its emulation reached 0.51 of the dv bound.  Neither is to be "aligned" with the other.)
    E_V(j,d)  = sum_i p_ij (e_p + u_p + n_j u) |dout_id|
        p rounded to bf16 before P^T dO (:638, :1197), fp32 accumulation over the key's n_j queries.
    E_K~(j,d) = sum_i (E_S + (u_s + n_j u) |dS_ij|) |q~_id| / sqrt D        E_Q~(i,d) likewise over j with k~ and n_i
        the rounding of the rotated q / k operand of the second product and the accumulation over the contributing rows.
    un-rotation on store (store_grad_unrot, attn_mfma.hip:191, :207-208; unrot_elem, attn_ref.hip:15-16): g_d c + g_d' s in fp32:
        E(d) = |c| E~(d) + |s| E~(d') + 2 u (|g~_d c| + |g~_d' s|)  on the rotary dims, E~(d) on the plain ones.
    bound = 4 * E + half an ulp of the output dtype.   The fixed factor 4 is the forward's: second-order products and the error of
        the normaliser that lse_i carries.
    bound_delta = D u sum_d |dout_id out_id| + half an fp32 ulp (attn_mfma.hip:521, :1017; attn_ref.hip:68).

The column sums of dqkv (``colsum``) are held to the sum of the column's per-element bounds plus rows * u * (sum_rows |dqkv| + |start|)
for their own fp32 accumulation over the B * S rows (attn_mfma.hip:1075, :1081, :1234, :1242; mafed_colsum).

The second half holds the case list, the input families and the dout rows of tests/test_gpu_attn_train_oracle.py; the CPU headroom
check and the guard of tests/test_attn_train_ref.py import the same generators."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from tests import attn_infer_ref as A
from tests.attn_infer_ref import Group, PathTerms, _rotate, attend, kernel_tables, make_rows, rnd, tables, ulp_out  # noqa: F401

F64 = torch.float64
U24 = A.U24
DTYPES = A.DTYPES
LAZY = 8.0 * math.log(2.0)

# attn_mfma.hip:731-735 rot_apply rotates the staged K rows in fp32 and packs them to bf16, :165-166 col_raw_finish does the same for q;
# :901, :906 pack_acc rounds p to bf16 for P V and for the ones-row sum alike; :900 v_exp_f32 (1 ulp) of s * scale2 - m, one fma or a
# product and a subtraction, with |s scale2 - m| <= (Delta + lazy) log2 e because the reference m is moved lazily (:889)
RESIDENT = PathTerms(A._FP32_ROT + A._BF16_ROT, 2.0 ** -9, 2 * U24 + 2.5 * U24 * LAZY, 2.5 * U24)
PATHS: Dict[str, PathTerms] = {"mfma": A.PATHS["mfma"], "exact-row": A.PATHS["exact-row"], "resident": RESIDENT}

# The backward's terms.  bf16 keeps 8 significant bits, so rounding to it moves a value just above a power of two by up to 2^-8 of
# itself (2^-9 only just below the next one): the backward's sums are held to that unit roundoff, for the rotated q / k operands
# (load_chunk_rot :65, rot_apply :734-735, col_raw_finish :166) and for p and dS (pack_acc :559, :638-639, :1054, :1197).  The
# exponential: __expf(s * scale - L) on the tiled kernels (:551, :632), v_exp_f32(s * scale2 - L * log2 e) on the resident ones
# (:1044-1050, :1185): one ulp of the hardware exp2, and two products and a subtraction at the magnitude |s| + |lse|.
BF16_U = 2.0 ** -8
BWD_PATHS: Dict[str, PathTerms] = {
    "mfma": PathTerms(A._FP32_ROT + BF16_U, BF16_U, *A._FAST_EXPF),
    "resident": PathTerms(A._FP32_ROT + BF16_U, BF16_U, *A._FAST_EXPF),
    # attn_ref.hip:65, :82, :130, :140 rot_elem in fp32; :85, :144 expf(s * scale - lse); sc / pq / dsq stay fp32
    "exact-row": A.PATHS["exact-row"],
}


# ------------------------------------------------------------------------------------------------------------------------------
# dispatch (attn.hip: mfma_ok; attn_mfma.hip: attn_resident_fits, attn_fwd_waves, mafed_attn_set_variant)
# ------------------------------------------------------------------------------------------------------------------------------
def resident_fits(S: int, D: int, rot: int = 0) -> bool:
    """the resident kernels rotate the column operand's first 32 dims only: 64 rotary dims go to the tiled kernels"""
    nrows = (S + 31) // 32 * 32
    return D <= 128 and rot <= 32 and nrows * D * 2 * 2 + nrows * 4 * 2 + D * 4 * 2 <= 160 * 1024


def fwd_waves(D: int) -> int:
    return 8 if D == 64 else 4


# ------------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------------
def visibility(S: int, P: int, am: Optional[torch.Tensor], B: int, causal: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(causal [S,S], pad [B,S]): key j of sample b is padded iff P <= j and am[b, j - P] == 0"""
    c = torch.ones(S, S, dtype=torch.bool)
    if causal:
        c = torch.tril(c)
    pad = torch.zeros(B, S, dtype=torch.bool)
    if am is not None and S > P:
        pad[:, P:] = am == 0
    return c, pad


def groups(qkv: torch.Tensor, causal: torch.Tensor, pad: torch.Tensor) -> List[Group]:
    """qkv [B,S,H,3,D] (fp64): one Group per sample, every row a query at its own position, every key rotated by the kernel"""
    B, S = qkv.shape[:2]
    pos = torch.arange(S)
    return [Group(q=qkv[b, :, :, 0], qpos=pos, k=qkv[b, :, :, 1], kpos=pos, krot=torch.ones(S, dtype=torch.bool), v=qkv[b, :, :, 2],
                  causal=causal, pad=pad[b]) for b in range(B)]


def forward_of(gs: List[Group], cos, sin) -> Dict[str, torch.Tensor]:
    """out, A [B*S,H,D]; sigma, delta [B*S,H]; nk [B*S] (attn_infer_ref.bound's quantities); lse, m, L [B,H,S]"""
    res = [A.solve(g, cos, sin) for g in gs]
    f = A._stack(res)
    f["res"] = res
    f["m"] = torch.stack([r["m"] for r in res])
    f["L"] = torch.stack([r["L"] for r in res])
    f["lse"] = f["m"] + f["L"].log()
    return f


def forward(qkv, causal, pad, cos, sin) -> Dict[str, torch.Tensor]:
    return forward_of(groups(qkv, causal, pad), cos, sin)


def rel_p(f: Dict[str, torch.Tensor], path: str) -> torch.Tensor:
    """the relative error of a row's p_j (the bracket of attn_infer_ref.bound, with this module's path terms) [B*S,H]"""
    t = PATHS[path]
    D = f["out"].shape[-1]
    return 2 * t.u_s * f["sigma"] + (t.exp_a + t.exp_b * f["delta"]) + t.u_p + (f["nk"].double()[:, None] + D) * U24


def out_bound(f, path: str, dtype: torch.dtype) -> torch.Tensor:
    """attn_infer_ref.bound's formula; the terms come from PATHS here, so that attn_infer_ref's table stays as it is"""
    return 4 * rel_p(f, path)[..., None] * f["A"] + ulp_out(f["out"], dtype)


def lse_bound(f, path: str) -> torch.Tensor:
    B, H, S = f["lse"].shape
    rel = rel_p(f, path).reshape(B, S, H).transpose(1, 2)
    lazy = LAZY if path == "resident" else 0.0
    return 4 * rel + 4 * U24 * (f["m"].abs() + f["L"].log().abs() + 2 * lazy) + ulp_out(f["lse"], torch.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------
def _rot_rows(x: torch.Tensor, cos, sin, shift: int = 0, inverse: bool = False) -> torch.Tensor:
    """x [B,S,H,D] rotated (or un-rotated) for position row + shift"""
    B, S, H, D = x.shape
    pos = (torch.arange(S) + shift).repeat(B)
    return _rotate(x.reshape(B * S, H, D), pos, cos, sin, inverse=inverse).reshape(B, S, H, D)


def backward(qkv, out, dout, lse, vis, cos, sin, *, delta=None, unrot_shift: int = 0, unrot_forward: bool = False,
             ds_scale: bool = True) -> Dict[str, torch.Tensor]:
    """qkv [B,S,H,3,D], out / dout [B,S,H,D], lse [B,H,S] (all fp64 values the kernel's dtypes hold), vis [B,S,S] -> dq, dk, dv
    [B,S,H,D], delta [B,H,S], colsum [3 H D] (the column sums of dqkv [B*S, H*3*D]) and the intermediates the bound is made of.  The
    keyword arguments are the guard's mutations: another delta, the un-rotation at position + shift or with the forward rotation, dS
    without its 1 / sqrt D."""
    B, S, H, _, D = qkv.shape
    qr, kr, v = _rot_rows(qkv[:, :, :, 0], cos, sin), _rot_rows(qkv[:, :, :, 1], cos, sin), qkv[:, :, :, 2]
    r = 1.0 / math.sqrt(D)
    s = torch.einsum("bihd,bjhd->bhij", qr, kr) * r
    p = torch.where(vis[:, None], (s - lse[..., None]).exp(), torch.zeros((), dtype=F64))
    dl = torch.einsum("bihd,bihd->bhi", dout, out)
    dP = torch.einsum("bihd,bjhd->bhij", dout, v)
    g = dP - (dl if delta is None else delta)[..., None]
    dS = p * g
    dv = torch.einsum("bhij,bihd->bjhd", p, dout)
    r2 = r if ds_scale else 1.0
    dkr = torch.einsum("bhij,bihd->bjhd", dS, qr) * r2
    dqr = torch.einsum("bhij,bjhd->bihd", dS, kr) * r2
    dq = _rot_rows(dqr, cos, sin, unrot_shift, inverse=not unrot_forward)
    dk = _rot_rows(dkr, cos, sin, unrot_shift, inverse=not unrot_forward)
    dqkv = torch.stack([dq, dk, dv], dim=3)
    return {"dq": dq, "dk": dk, "dv": dv, "delta": dl, "dqkv": dqkv, "colsum": dqkv.reshape(B * S, H * 3 * D).sum(dim=0),
            "qr": qr, "kr": kr, "s": s, "p": p, "g": g, "dS": dS, "dqr": dqr, "dkr": dkr}


def _rot_mag(x: torch.Tensor, cos, sin) -> torch.Tensor:
    """|x c| + |y s| of every rotated element of rows x [B,S,H,D] (|x| on the plain dims): what the rotation's roundings scale with,
    which the rotated element itself may be far smaller than"""
    S, rot = x.shape[1], cos.shape[1]
    a = x.abs()
    if rot == 0:
        return a
    half = rot // 2
    c, s = cos.double().abs()[:S, None, :], sin.double().abs()[:S, None, :]
    out = a.clone()
    out[..., :rot] = a[..., :rot] * c + torch.cat([a[..., half:rot], a[..., :half]], dim=-1) * s
    return out


def _unrot_err(E: torch.Tensor, G: torch.Tensor, cos, sin) -> torch.Tensor:
    """error of the un-rotated row from the error E and the value G of the rotated-frame row, [B,S,H,D]"""
    S, rot = E.shape[1], cos.shape[1]
    if rot == 0:
        return E
    half = rot // 2
    c, s = cos.double().abs()[:S, None, :], sin.double().abs()[:S, None, :]
    swap = lambda x: torch.cat([x[..., half:rot], x[..., :half]], dim=-1)
    out = E.clone()
    out[..., :rot] = c * E[..., :rot] + s * swap(E) + 2 * U24 * (c * G[..., :rot].abs() + s * swap(G.abs()))
    return out


def backward_bound(qkv, out, dout, lse, vis, cos, sin, r: Dict[str, torch.Tensor], path: str, dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    """per-element bounds of dq, dk, dv [B,S,H,D], of delta [B,H,S] and of colsum [3 H D] given a start value of magnitude 0 (the
    caller adds rows * u * |start|): the module docstring, term by term"""
    t = BWD_PATHS[path]
    B, S, H, _, D = qkv.shape
    rs = 1.0 / math.sqrt(D)
    qa, ka = _rot_mag(qkv[:, :, :, 0], cos, sin), _rot_mag(qkv[:, :, :, 1], cos, sin)
    va, da = qkv[:, :, :, 2].abs(), dout.abs()
    sabs = torch.einsum("bihd,bjhd->bhij", qa, ka) * rs
    p, g, dSa = r["p"], r["g"].abs(), r["dS"].abs()
    e_p = (2 * t.u_s + D * U24) * sabs + t.exp_a + t.exp_b * (r["s"].abs() + lse.abs()[..., None])
    aD = torch.einsum("bihd,bihd->bhi", da, out.abs())
    e_d = D * U24 * (torch.einsum("bihd,bjhd->bhij", da, va) + aD[..., None]) + U24 * g
    E_S = p * (e_p * g + e_d) + (t.u_p + 3 * U24) * dSa
    n_i = vis.sum(dim=2).double()[:, :, None, None]      # keys of row i      [B,S,1,1]
    n_j = vis.sum(dim=1).double()[:, :, None, None]      # queries of key j
    E_V = torch.einsum("bhij,bihd->bjhd", p * (e_p + t.u_p), da) + n_j * U24 * torch.einsum("bhij,bihd->bjhd", p, da)
    E_K = (torch.einsum("bhij,bihd->bjhd", E_S, qa) + (t.u_s + n_j * U24) * torch.einsum("bhij,bihd->bjhd", dSa, qa)) * rs
    E_Q = (torch.einsum("bhij,bjhd->bihd", E_S, ka) + (t.u_s + n_i * U24) * torch.einsum("bhij,bjhd->bihd", dSa, ka)) * rs
    b = {"dq": 4 * _unrot_err(E_Q, r["dqr"], cos, sin) + ulp_out(r["dq"], dtype),
         "dk": 4 * _unrot_err(E_K, r["dkr"], cos, sin) + ulp_out(r["dk"], dtype),
         "dv": 4 * E_V + ulp_out(r["dv"], dtype),
         "delta": D * U24 * aD + ulp_out(r["delta"], torch.float32)}
    per = torch.stack([b["dq"], b["dk"], b["dv"]], dim=3).reshape(B * S, H * 3 * D)
    b["colsum"] = per.sum(dim=0) + B * S * U24 * r["dqkv"].reshape(B * S, H * 3 * D).abs().sum(dim=0)
    return b


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    op: str                 # causal | bidir
    dtype: str              # f32 | bf16
    D: int
    H: int
    S: int
    T: int                  # text positions (P = S - T image keys in front); bidir: 0
    pads: Tuple[int, ...]   # left padding of every sample's text; len = B
    rot: int = -1           # -1: D // 4
    variant: int = 0        # mafed_attn_set_variant: 1 = the tiled kernels even where the resident ones fit
    exact: bool = False     # bf16 forward through ops.attn_fwd_exact_bf16 (the row kernel on MFMA shapes); no backward
    note: str = ""

    @property
    def B(self):
        return len(self.pads)

    @property
    def P(self):
        return self.S - self.T

    @property
    def rotary(self):
        return 0 if self.op == "bidir" else (self.D // 4 if self.rot < 0 else self.rot)

    @property
    def causal(self):
        return self.op == "causal"

    @property
    def path(self) -> str:
        if self.dtype == "f32" or self.exact:
            return "exact-row"
        if self.op == "bidir":
            assert self.D == 64 and resident_fits(self.S, self.D), "attn_fwd_bidir (bf16) has the resident D = 64 kernel only"
            return "resident"
        if not A.mfma_ok(self.D, self.rotary):
            return "exact-row"
        return "resident" if self.variant == 0 and resident_fits(self.S, self.D, self.rotary) else "mfma"

    @property
    def backward(self) -> bool:
        return self.causal and not self.exact

    @property
    def label(self) -> str:
        """the path as the commit message lists it"""
        if self.op == "bidir":
            return "bidirectional"
        if self.path == "exact-row":
            return "exact-row " + ("fp32" if self.dtype == "f32" else "bf16")
        return ("resident" if self.path == "resident" else "tiled") + f" D={self.D}"

    @property
    def id(self) -> str:
        s = f"{self.op}-{self.dtype}-D{self.D}r{self.rotary}-B{self.B}H{self.H}-S{self.S}T{self.T}"
        return s + ("-tiled" if self.variant else "") + ("-exact" if self.exact else "")


def _c(D, S, T, pads=None, H=1, **kw) -> Case:
    if pads is None:
        pads = (0, min(3, T - 1), T - 1)
    return Case(op="causal", dtype=kw.pop("dtype", "bf16"), D=D, H=H, S=S, T=T, pads=pads, **kw)


def cases() -> List[Case]:
    c: List[Case] = []
    # resident, D = 64: 8 forward waves, 4 backward waves; rounds of 8 / 4 slices of 16 rows
    c.append(_c(64, 7, 3, H=2, note="one ragged slice, every other wave idle"))
    c.append(_c(64, 33, 9, H=2, note="three slices: less than one round"))
    c.append(_c(64, 64, 10, H=2, note="one key tile exactly"))
    c.append(_c(64, 65, 10, H=2, note="one key into the second tile"))
    c.append(_c(64, 129, 1, pads=(0, 0), H=2, note="T = 1"))
    c.append(_c(64, 288, 32, H=2, note="the training shape: P = 256, T = 32"))
    c.append(_c(64, 608, 40, pads=(0, 39), note="the last resident S at D = 64"))
    # resident, D = 128
    c.append(_c(128, 40, 8))
    c.append(_c(128, 257, 20, pads=(0, 19)))
    c.append(_c(128, 288, 32, pads=(0, 31), note="the last resident S at D = 128"))
    # tiled by size
    c.append(_c(64, 609, 40, pads=(0, 39), note="the first tiled S at D = 64"))
    c.append(_c(64, 641, 70, pads=(0, 69), note="eleven tiles, one row in the last"))
    c.append(_c(128, 289, 33, pads=(0, 32), note="the first tiled S at D = 128"))
    c.append(_c(256, 14, 5, pads=(0, 4)))
    c.append(_c(256, 83, 20, pads=(0, 19), note="P = 63"))
    c.append(_c(256, 288, 32, pads=(0, 31)))
    # tiled by variant 1 on resident shapes
    for D in (64, 128):
        c.append(_c(D, 65, 10, H=2 if D == 64 else 1, variant=1))
        c.append(_c(D, 288, 32, pads=(0, 31), variant=1))
    # P against the 64-key tile: the plain / masked tile split (kt_plain, need_mask)
    for P in (63, 64, 65):
        c.append(_c(64, P + 70, 70, note=f"P = {P}"))
    c.append(_c(64, 70, 70, pads=(0, 0), note="P = 0, no padding"))
    # rotary dims on the MFMA paths (rot = 16 at D = 64 and 32 at D = 128 are the default above); rot = D once
    c.append(_c(64, 81, 12, rot=0))
    c.append(_c(64, 81, 12, rot=32))
    c.append(_c(64, 81, 12, rot=64, note="rot = D; 64 rotary dims: tiled"))
    c.append(_c(128, 40, 8, rot=16))
    c.append(_c(128, 40, 8, rot=64, note="64 rotary dims: tiled"))
    c.append(_c(256, 40, 8, rot=16, pads=(0, 7)))
    # bf16 without an MFMA kernel (mfma_ok), fp32: the row kernels
    c.append(_c(64, 33, 9, rot=20, H=2))
    c.append(_c(80, 70, 7, rot=20))
    c.append(_c(64, 65, 10, H=2, dtype="f32"))
    c.append(_c(80, 33, 9, dtype="f32"))
    c.append(_c(256, 14, 5, pads=(0, 4), dtype="f32"))
    # the row kernel on bf16 data at an MFMA shape (forward only)
    c.append(_c(64, 65, 10, H=2, exact=True))
    c.append(_c(128, 40, 8, exact=True))
    # bidirectional (CLIP tower): forward only
    for S in (40, 128, 257):
        c.append(Case(op="bidir", dtype="bf16", D=64, H=2, S=S, T=0, pads=(0, 0)))
    c.append(Case(op="bidir", dtype="f32", D=64, H=2, S=40, T=0, pads=(0, 0)))
    c.append(Case(op="bidir", dtype="f32", D=80, H=1, S=33, T=0, pads=(0, 0)))
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
# "gentle": the ascending rows with q / 16, so that |s| stays below 2.  With bf16 operands at |s| = 30 the bound's 2 u_s sabs term alone
# allows a p_ij half of itself, and one term of a dQ / dK sum is no larger than the sum's bound; at |s| <= 2 a single dropped key or
# query shows, and unlike the census family (q = 0: dK = 0) every gradient is there.  The hot query moves over the edges as in peaked.
FAMILIES = A.FAMILIES + ("gentle",)
HOT_DOUT = 64.0    # the hot query's dout row is this much larger: against 4 * 2 * 2^-8 of the sum of a key's 600 other queries it still shows


def dout_kind(fam: str) -> str:
    """census and masked-max count queries (one-hot dout rows), the others carry a bit-hash row"""
    return "census" if fam in ("census", "masked-max") else "hash"


def hot_rows(case: Case) -> List[int]:
    """peaked: where the hot key (and the hot query) sits, in turn: 0, the slice edge 15 / 16, the tile edge 63 / 64, P - 1, P (a padded
    P moves to the sample's first visible text key), one row inside the text, S - 1.  Key j is on the diagonal of row j."""
    S, P = case.S, case.P
    e = {0, 15, 16, 63, 64, S - 1}
    if case.causal:
        e |= {P - 1, P, P + max(case.pads), (P + S) // 2}
    return sorted(j for j in e if 0 <= j < S)


def variants(case: Case, fam: str) -> List[Optional[int]]:
    return hot_rows(case) if fam in ("peaked", "gentle") else [None]


def resolve_hot(case: Case, b: int, j: Optional[int]) -> int:
    if j is None:
        return -1
    return case.P + case.pads[b] if case.causal and case.P <= j < case.P + case.pads[b] else j


def _rows(fam, H, D, rot, pos, order, hot, masked, code, cos, sin):
    if 0 < rot < D:
        return make_rows(fam, H, D, rot, pos, order, hot, masked, code, cos, sin)
    # make_rows wants a rotary pair and a plain dim behind it to put the score design on; rot = 0 has no pair and rot = D no plain dim.
    # Take its rotated-frame design for 16 rotary dims (identity tables: nothing is un-rotated) and un-rotate q and k with the real
    # tables (nothing to do at rot = 0), so that the kernel's rotation at the right position restores that design
    one, zero = torch.ones(cos.shape[0], 16), torch.zeros(cos.shape[0], 16)
    rows = make_rows(fam, H, D, 16, pos, order, hot, masked, code, one, zero)
    p = torch.as_tensor(pos)
    rows[:, :, 0] = _rotate(rows[:, :, 0], p, cos, sin, inverse=True)
    rows[:, :, 1] = _rotate(rows[:, :, 1], p, cos, sin, inverse=True)
    return rows


def make_dout(kind: str, B: int, S: int, H: int, D: int, hot: List[int]) -> torch.Tensor:
    """[B,S,H,D] fp64.  census: 1 at d = code mod D, so dV_j counts the queries that reached key j; hash: +-1/8 by one bit of a hash of
    (code, head, d), so that dP - delta is O(1).  code = row + 101 b + 53 h; the hot row of a sample is HOT_DOUT times larger."""
    code = (torch.arange(S)[None, :, None] + 101 * torch.arange(B)[:, None, None] + 53 * torch.arange(H)[None, None, :])[..., None]
    d = torch.arange(D)[None, None, None, :]
    if kind == "census":
        x = (code % D == d).double()
    else:
        z = ((code + 7) * 2246822519 + (d + 3) * 2654435761) % (1 << 32)
        z = ((z ^ (z >> 13)) * 2654435761) % (1 << 32)
        x = (((z >> 11) & 1).double() * 2 - 1) * 0.125
    x = x.expand(B, S, H, D).clone()
    for b, j in enumerate(hot):
        if j >= 0:
            x[b, j] *= HOT_DOUT
    return x


def build(case: Case, fam: str, hot: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """What the kernels read, as fp64 values the case's dtype holds exactly: qkv [B,S,H,3,D], dout [B,S,H,D], am [B,T], the oracle's
    rotary tables, causal [S,S], pad [B,S], vis [B,S,S]."""
    B, H, D, S, P, T, rot = case.B, case.H, case.D, case.S, case.P, case.T, case.rotary
    cos, sin = tables(D, rot, S + 2)
    am = torch.ones(B, T, dtype=torch.int64)
    for b in range(B):
        am[b, : case.pads[b]] = 0
    causal, pad = visibility(S, P, am if case.causal else None, B, case.causal)
    pos = torch.arange(S)
    hots = [resolve_hot(case, b, hot) for b in range(B)]
    qkv = torch.stack([rnd(_rows("ascending" if fam == "gentle" else fam, H, D, rot, pos, pos.double() / max(1, S - 1), pos == hots[b], pad[b], pos + 101 * b, cos, sin), case.dtype)
                       for b in range(B)])
    if fam == "gentle":
        qkv[:, :, :, 0] /= 16.0
    if not case.causal:
        # every bidirectional row sees every key, and make_rows gives every row the same query: row i gets 1, 1/2 or 1/4 of it, so that
        # neighbouring rows differ in out and lse
        qkv[:, :, :, 0] *= (0.5 ** (pos % 3).double())[None, :, None, None]
    dout = rnd(make_dout(dout_kind(fam), B, S, H, D, hots), case.dtype)
    return {"qkv": qkv, "dout": dout, "am": am, "cos": cos, "sin": sin, "causal": causal, "pad": pad,
            "vis": causal[None] & ~pad[:, None, :], "hot": hots}


def handed_over(case: Case, f: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """out [B,S,H,D] and lse [B,H,S] as the backward is handed them: the fp64 forward rounded to the dtype and to fp32"""
    out = rnd(f["out"].reshape(case.B, case.S, case.H, case.D), case.dtype)
    return out, f["lse"].float().double()
