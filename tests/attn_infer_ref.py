"""fp64 reference of the inference attention kernels, stated at the kernels' interface, with the error bound their outputs are held
to and the inputs that make a wrong key visible.  Plain torch, CPU; nothing here imports ``mafed_amd`` and nothing calls ``attn_fwd``.

Every kernel of this family computes, for a query row and a head,

    out_d = sum_j p_j v_jd,   p_j = exp(s_j - m) / sum_j' exp(s_j' - m),   s_j = <rot(q), rot(k_j)> / sqrt(D)

over the keys j the row may see.  The kernels differ in where the keys live (prefill cache, generated rows, beam slots, image store,
candidates), in which keys they rotate themselves, and in where they round.  The first is the business of ``decode`` / ``decode_beam`` /
``suffix`` / ``cand`` below: each turns the tensors a kernel reads (already rounded to the kernel's dtype and up-cast) into one
``Group`` per independent key axis and solves it in fp64.  The last is the business of ``PATHS`` and ``bound``.

The error model (first order, per output element; u = 2^-24):

    bound_d = 4 * (2 u_s sigma + u_exp(Delta) + u_p + (nk + D) u) * A_d + ulp_out(out_d)

  * a relative rounding u_s of the rotated q and of the rotated k moves a score by at most 2 u_s sigma, sigma = max_j sum_d |q_d k_jd| /
    sqrt(D), and so moves p_j by that fraction of itself;
  * the exponential carries its own relative error plus that of its argument, which grows with |s_j - m| <= Delta:
    u_exp(Delta) = exp_a + exp_b * Delta;
  * u_p is the rounding of p before the PV product (bf16 MFMA operand), 0 where p stays in fp32;
  * (nk + D) u stands for the fp32 accumulation chains: D terms under a score, nk (visible keys) under the V sum and the row sum, and
    the rescalings of the online forms, of which there are fewer than nk / 8 per state;
  * all of these are relative errors of the p_j, so they move out_d by at most that fraction of A_d = sum_j p_j |v_jd|; the same
    fraction of the normaliser is a second term of at most the same size, the products of two errors are second order: the fixed
    factor 4 covers both;
  * ulp_out is half an ulp of the output dtype at out_d: the final rounding.

The second half of the file holds the input families and the case list of tests/test_gpu_attn_infer_oracle.py; the CPU guard of
tests/test_attn_infer_ref.py imports the same generators, so what runs on the GPU is what was shown to be sharp enough."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from oracle import vlpythia_ref as R

F64 = torch.float64
U24 = 2.0 ** -24
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


# ------------------------------------------------------------------------------------------------------------------------------
# rotary tables and the rotation (oracle.vlpythia_ref: rotary_tables, apply_partial_rotary)
# ------------------------------------------------------------------------------------------------------------------------------
def tables(D: int, rot: int, S: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The oracle's fp32 cos / sin tables [S, rot] for a head of D dims of which the first ``rot`` rotate."""
    cfg = R.RefConfig(hidden_size=D, num_attention_heads=1, rotary_pct=rot / D)
    assert cfg.rotary_ndims == rot, (D, rot, cfg.rotary_ndims)
    return R.rotary_tables(cfg, S)


def kernel_tables(cos: torch.Tensor, sin: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The [S, rot / 2] halves the kernels take (the oracle's tables repeat them)."""
    half = cos.shape[1] // 2
    return cos[:, :half].contiguous(), sin[:, :half].contiguous()


def _rotate(x: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Rows x [n, H, D] (fp64) rotated for positions pos [n]; ``inverse`` undoes it."""
    c, s = cos.double()[pos], sin.double()[pos]
    if inverse:
        s = -s
    return R.apply_partial_rotary(x.transpose(0, 1)[None], c, s)[0].transpose(0, 1)


def rotate_k(qkv: torch.Tensor, S: int, H: int, D: int, rot: int, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """The k third of every row of a [.., S, H, 3, D] tensor rotated for its position (row index within the sample); q and v as given."""
    x = qkv.double().reshape(-1, S, H, 3, D).clone()
    pos = torch.arange(S).repeat(x.shape[0])
    x[:, :, :, 1] = _rotate(x[:, :, :, 1].reshape(-1, H, D), pos, cos, sin).reshape(-1, S, H, D)
    return x.reshape(qkv.shape)


def rotate_k_operands(qkv: torch.Tensor, S: int, H: int, D: int, rot: int, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """|x c| + |y s| of every rotated element of the k third (|x| for the others): the magnitude the rotation's roundings scale with."""
    k = qkv.double().reshape(-1, S, H, 3, D)[:, :, :, 1].abs()
    half = rot // 2
    c, s = cos.double().abs()[:S, None, :], sin.double().abs()[:S, None, :]
    m = k.clone()
    m[..., :rot] = k[..., :rot] * c + torch.cat([k[..., half:rot], k[..., :half]], dim=-1) * s
    return m


# ------------------------------------------------------------------------------------------------------------------------------
# one key axis, solved in fp64
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Group:
    """Queries that share one key axis.  q [Rq,H,D] at positions qpos, keys k / v [nk,H,D] at positions kpos; krot[j]: key j arrives
    un-rotated (the kernel rotates it at kpos[j]), else it is used as stored; causal [Rq,nk]: key j lies in row r's range; pad [nk]: key
    j is a padded text key.  A row sees causal & ~pad."""
    q: torch.Tensor
    qpos: torch.Tensor
    k: torch.Tensor
    kpos: torch.Tensor
    krot: torch.Tensor
    v: torch.Tensor
    causal: torch.Tensor
    pad: torch.Tensor

    def vis(self) -> torch.Tensor:
        return self.causal & ~self.pad[None, :]


def attend(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, vis: torch.Tensor) -> Dict[str, torch.Tensor]:
    """softmax(q k^T / sqrt D) v over the visible keys, with what the bound needs.  q [Rq,H,D], k / v [nk,H,D] (as the dot product sees
    them), vis [Rq,nk] ->  out, A [Rq,H,D]; sigma, delta [Rq,H]; nk [Rq]; p, s [H,Rq,nk]; m, L [H,Rq]."""
    D = q.shape[-1]
    assert bool(vis.any(dim=1).all()), "a query row without a visible key"
    vb = vis[None]
    s = torch.einsum("rhd,jhd->hrj", q, k) / math.sqrt(D)
    sabs = torch.einsum("rhd,jhd->hrj", q.abs(), k.abs()) / math.sqrt(D)
    m = s.masked_fill(~vb, -math.inf).amax(dim=-1)
    w = torch.where(vb, (s - m[..., None]).clamp(max=0.0).exp(), torch.zeros((), dtype=F64))
    L = w.sum(dim=-1)
    p = w / L[..., None]
    return {
        "out": torch.einsum("hrj,jhd->rhd", p, v), "A": torch.einsum("hrj,jhd->rhd", p, v.abs()),
        "sigma": sabs.masked_fill(~vb, 0.0).amax(dim=-1).transpose(0, 1), "delta": (m[..., None] - s).masked_fill(~vb, 0.0).amax(dim=-1).transpose(0, 1),
        "nk": vis.sum(dim=1), "p": p, "s": s, "m": m, "L": L,
    }


def rotated_keys(g: Group, cos, sin) -> torch.Tensor:
    return torch.where(g.krot[:, None, None], _rotate(g.k, g.kpos, cos, sin), g.k)


def solve(g: Group, cos, sin) -> Dict[str, torch.Tensor]:
    return attend(_rotate(g.q, g.qpos, cos, sin), rotated_keys(g, cos, sin), g.v, g.vis())


def _stack(res: List[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
    out = {key: torch.cat([r[key] for r in res], dim=0) for key in ("out", "A", "sigma", "delta", "nk")}
    out["p"] = [r["p"] for r in res]
    return out


def _pad_keys(am_b: Optional[torch.Tensor], P: int, S0: int, n: int) -> torch.Tensor:
    """key j of a [P image | S0 - P text | ...] axis of n keys is padded iff P <= j < S0 and am[j - P] == 0"""
    pad = torch.zeros(n, dtype=torch.bool)
    if S0 > P:
        pad[P:S0] = am_b[: S0 - P] == 0
    return pad


# ------------------------------------------------------------------------------------------------------------------------------
# the four kernels' interfaces
# ------------------------------------------------------------------------------------------------------------------------------
def decode_groups(prefix, new, t, am, P, prerot) -> List[Group]:
    """prefix [B,S0,H,3,D], new [B,cap,H,3,D]: one query per sample, row t of ``new`` at position S0 + t, keys 0 .. S0 + t."""
    B, S0 = prefix.shape[:2]
    n = S0 + t + 1
    out = []
    for b in range(B):
        rows = torch.cat([prefix[b], new[b, : t + 1]], dim=0).double()
        krot = torch.full((n,), not prerot, dtype=torch.bool)
        krot[n - 1] = True    # row t always arrives un-rotated
        out.append(Group(q=rows[n - 1:, :, 0], qpos=torch.tensor([S0 + t]), k=rows[:, :, 1], kpos=torch.arange(n), krot=krot, v=rows[:, :, 2],
                         causal=torch.ones(1, n, dtype=torch.bool), pad=_pad_keys(am[b], P, S0, n)))
    return out


def decode(prefix, new, t, am, P, rot, cos, sin, prerot=False):
    """One decode step.  Keys 0 .. S0 + t are visible iff j < P or j >= S0 or am[b, j - P] != 0.  prerot: the prefix and rows < t of
    ``new`` hold rotated keys as given, row t is un-rotated; the rotated key of row t is returned too (``k_t`` [B,H,D])."""
    groups = decode_groups(prefix, new, t, am, P, prerot)
    res = _stack([solve(g, cos, sin) for g in groups])
    if prerot:
        res["k_t"] = torch.stack([rotated_keys(g, cos, sin)[-1] for g in groups])
    return res


def decode_beam_groups(prefix, new, anc, t, k, am, P) -> List[Group]:
    """prefix [B,S0,H,3,D] (rotated keys), new [B*k,cap,H,3,D], anc [B*k,cap]: beam r reads row j < t from slot anc[r, j] (rotated) and
    row t from its own slot (un-rotated)."""
    B, S0 = prefix.shape[:2]
    n = S0 + t + 1
    out = []
    for r in range(B * k):
        b = r // k
        hist = [new[int(anc[r, j]), j] for j in range(t)] + [new[r, t]]
        rows = torch.cat([prefix[b], torch.stack(hist)], dim=0).double()
        krot = torch.zeros(n, dtype=torch.bool)
        krot[n - 1] = True
        out.append(Group(q=rows[n - 1:, :, 0], qpos=torch.tensor([S0 + t]), k=rows[:, :, 1], kpos=torch.arange(n), krot=krot, v=rows[:, :, 2],
                         causal=torch.ones(1, n, dtype=torch.bool), pad=_pad_keys(am[b], P, S0, n)))
    return out


def decode_beam(prefix, new, anc, t, k, am, P, rot, cos, sin):
    groups = decode_beam_groups(prefix, new, anc, t, k, am, P)
    res = _stack([solve(g, cos, sin) for g in groups])
    res["k_t"] = torch.stack([rotated_keys(g, cos, sin)[-1] for g in groups])
    return res


def suffix_groups(qkv_img, image_index, qkv_txt, am) -> List[Group]:
    """qkv_img [N,P,H,3,D], qkv_txt [B,T,H,3,D]: text row q of prompt b sits at position P + q and sees the P keys of image
    image_index[b] and the text keys 0 .. q of its prompt that the mask leaves (its own key too only if the mask leaves it)."""
    P = qkv_img.shape[1]
    B, T = qkv_txt.shape[:2]
    n = P + T
    out = []
    for b in range(B):
        rows = torch.cat([qkv_img[int(image_index[b])], qkv_txt[b]], dim=0).double()
        qpos = P + torch.arange(T)
        out.append(Group(q=rows[P:, :, 0], qpos=qpos, k=rows[:, :, 1], kpos=torch.arange(n), krot=torch.ones(n, dtype=torch.bool), v=rows[:, :, 2],
                         causal=torch.arange(n)[None, :] <= qpos[:, None], pad=_pad_keys(am[b], P, n, n)))
    return out


def suffix(qkv_img, image_index, qkv_txt, am, rot, cos, sin):
    return _stack([solve(g, cos, sin) for g in suffix_groups(qkv_img, image_index, qkv_txt, am)])


def cand_groups(qkv_pre, qkv_cand, am) -> List[Group]:
    """qkv_pre [B,S0,H,3,D], qkv_cand [B,C,A,H,3,D], am [B,T] (None: T = 0): row i of candidate (b, c) sits at position S0 + i and
    sees the visible prefix keys and rows 0 .. i of its own candidate."""
    B, S0 = qkv_pre.shape[:2]
    C, A = qkv_cand.shape[1:3]
    T = 0 if am is None else am.shape[1]
    n = S0 + A
    out = []
    for b in range(B):
        for c in range(C):
            rows = torch.cat([qkv_pre[b], qkv_cand[b, c]], dim=0).double()
            qpos = S0 + torch.arange(A)
            out.append(Group(q=rows[S0:, :, 0], qpos=qpos, k=rows[:, :, 1], kpos=torch.arange(n), krot=torch.ones(n, dtype=torch.bool), v=rows[:, :, 2],
                             causal=torch.arange(n)[None, :] <= qpos[:, None], pad=_pad_keys(None if am is None else am[b], S0 - T, S0, n)))
    return out


def cand(qkv_pre, qkv_cand, am, rot, cos, sin):
    return _stack([solve(g, cos, sin) for g in cand_groups(qkv_pre, qkv_cand, am)])


# ------------------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class PathTerms:
    u_s: float     # relative rounding of a rotated q / k element before the score product
    u_p: float     # relative rounding of p before the PV product
    exp_a: float   # relative error of the exponential itself
    exp_b: float   # ... and per unit of |s - m|: the rounding of its argument


_FP32_ROT = 2 * U24        # x c -+ y s in fp32: two roundings, the result stays in fp32
_BF16_ROT = 2.0 ** -9      # ... then rounded to bf16: half an ulp of 8 significant bits
_EXPF = (2 * U24, U24)                # expf: 1 ulp; its argument s - m is one fp32 subtraction, |s - m| <= Delta
_FAST_EXPF = (2 * U24, 2.5 * U24)     # __expf = exp2(x * log2 e): 1 ulp of the hardware exp2; the subtraction, the product and the constant

PATHS: Dict[str, PathTerms] = {
    # attn_decode.hip:43 q = rot_elem() into LDS as fp32, :52 k = rot_elem() in fp32; :61 expf(sc[j] - m); :71 p stays fp32 under the V fma
    "scalar": PathTerms(_FP32_ROT, 0.0, *_EXPF),
    # attn_decode.hip:146 q = load_chunk_rot8 -> q_s fp32, :196 kr = x c + sgn y s in fp32; :205-206 expf; :209 fmaf(acc, corr, p * vv) in fp32
    "fused": PathTerms(_FP32_ROT, 0.0, *_EXPF),
    # attn_decode.hip:190 cache keys used as stored, row t from knew_s (fp32, :153); q as above; :205-206 expf; :209 p in fp32
    "fused-prerot": PathTerms(_FP32_ROT, 0.0, *_EXPF),
    # attn_decode.hip:293-294 q and row t's key rotated in fp32 registers, cache keys as stored; :331 __expf(sc[u] - mx); :334 p in fp32
    "flat": PathTerms(_FP32_ROT, 0.0, *_FAST_EXPF),
    # attn_decode_beam.hip:52 q_s = rotated q * scale in fp32, :55 knew_s fp32; :15-16 __expf in online_add (and :136, :161 in the merges); :19 p in fp32
    "beam": PathTerms(_FP32_ROT, 0.0, *_FAST_EXPF),
    # attn.h:51 k = rot_elem() in fp32 against qrow (attn_suffix.hip:32 / attn_cand.hip:32, fp32 in LDS); attn.h:60 expf; attn.h:69 p in fp32
    "exact-row": PathTerms(_FP32_ROT, 0.0, *_EXPF),
    # attn_mfma.hip:65 load_chunk_rot packs rotated q / k to bf16 for the MFMA; :293 pack_acc rounds p to bf16 before P V; :279, :286 __expf
    "mfma": PathTerms(_FP32_ROT + _BF16_ROT, 2.0 ** -9, *_FAST_EXPF),
}


def ulp_out(out: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Half an ulp of ``dtype`` at |out| (at the smallest normal number below it)."""
    bits = {torch.float32: 24, torch.bfloat16: 8}[dtype]
    _, e = torch.frexp(out.double().abs())     # |out| = mant * 2^e, mant in [0.5, 1): ulp = 2^(e - bits)
    e = torch.where(out == 0, torch.full_like(e, -125), e).clamp(min=-125)
    return torch.ldexp(torch.ones_like(out, dtype=F64), e - bits - 1)


def bound(quantities: Dict[str, torch.Tensor], path: str, out_dtype: torch.dtype) -> torch.Tensor:
    t = PATHS[path]
    out, A = quantities["out"], quantities["A"]
    D = out.shape[-1]
    sigma, delta = quantities["sigma"][..., None], quantities["delta"][..., None]
    nk = quantities["nk"].double()[:, None, None]
    rel = 2 * t.u_s * sigma + (t.exp_a + t.exp_b * delta) + t.u_p + (nk + D) * U24
    return 4 * rel * A + ulp_out(out, out_dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# which kernel a shape reaches (attn_decode.hip: attn_decode_launch; attn.hip: mfma_ok; attn_decode_beam.hip: attn_decode_beam_go)
# ------------------------------------------------------------------------------------------------------------------------------
def decode_path(dtype: str, D: int, rot: int, nk: int, Tm: int, prerot: bool, flat: bool) -> str:
    if rot % 16 == 0 and D in (64, 128, 256):
        if dtype == "bf16" and prerot and flat and Tm <= 256 and D in (64, 128):
            groups = 256 // (D // 8)
            if (nk + groups - 1) // groups <= 24:
                return "flat"
        return "fused-prerot" if prerot else "fused"
    assert not prerot
    return "scalar"


def mfma_ok(D: int, rot: int) -> bool:
    return D in (64, 128, 256) and rot in (0, 16, 32, 64) and rot <= D


def rows_path(dtype: str, D: int, rot: int) -> str:
    return "mfma" if dtype == "bf16" and mfma_ok(D, rot) else "exact-row"


def beam_kb(k: int) -> int:
    return 2 if k <= 2 else (4 if k <= 4 else 8)


# ------------------------------------------------------------------------------------------------------------------------------
# input families
# ------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("census", "peaked", "ascending", "descending", "masked-max")
HOT_GAIN = 6.0      # peaked: the hot key gains this much from the plain dims and as much again from the rotary pair it shares with q


def rnd(x: torch.Tensor, dtype: str) -> torch.Tensor:
    """x as the kernel will read it: rounded to the dtype, up-cast again"""
    return x.to(DTYPES[dtype]).double()


def make_rows(fam: str, H: int, D: int, rot: int, pos, order, hot, masked, code, cos, sin) -> torch.Tensor:
    """Fused q | k | v rows [n,H,3,D] (fp64, not yet rounded) of one family.  Per row: pos (rotary position), order in [0, 1] (where the
    row stands along its key axis: the score ramp), hot (peaked: this is the hot key), masked (a padded text key), code (an integer
    that names the row: V encodes it).  Scores are designed in the rotated frame and the rows un-rotated for their position, so the
    kernel's rotation at the right position restores the design and at any other does not.

      q: 0 for census.  Else 8 on the first plain dim, g on the first rotary pair, small texture elsewhere.
      k: score * sqrt(D) / 8 on the first plain dim; on the first rotary pair g aligned with q for the hot key (+ g^2 / sqrt D), g / 4 at
         a code-dependent angle for the others; small texture elsewhere.
      v: census: 1 at d = code mod D; else one bit of a 32-bit hash of (code + 1 + 37 h, d).  Masked rows: 1 everywhere."""
    n = len(pos)
    pos, order, code = torch.as_tensor(pos), torch.as_tensor(order, dtype=F64), torch.as_tensor(code)
    hot, masked = torch.as_tensor(hot, dtype=torch.bool), torch.as_tensor(masked, dtype=torch.bool)
    half = rot // 2
    hh = torch.arange(H)
    d = torch.arange(D)
    rows = torch.zeros(n, H, 3, D, dtype=F64)
    if fam == "census":
        v = (code[:, None, None] % D == d[None, None, :]).double().expand(n, H, D).clone()
    else:
        c = code[:, None] + 1 + 37 * hh[None, :]
        x = (c[:, :, None] * 2654435761 + (d[None, None, :] + 1) * 2246822519) % (1 << 32)    # a 32-bit hash of (code, head, d): rows with
        x = ((x ^ (x >> 15)) * 2246822519) % (1 << 32)                                         # neighbouring codes differ in about half the dims
        v = ((x >> 13) & 1).double()
    v[masked] = 1.0
    rows[:, :, 2] = v
    if fam == "peaked":
        base = torch.where(hot, torch.tensor(HOT_GAIN, dtype=F64), torch.zeros((), dtype=F64))
        g = math.sqrt(HOT_GAIN * math.sqrt(D))
    else:
        base = {"ascending": -30.0 + 60.0 * order, "descending": 30.0 - 60.0 * order}.get(fam, -30.0 + 60.0 * order)
        g = 1.0
    if fam == "masked-max":
        base = torch.where(masked, torch.tensor(40.0, dtype=F64), base)
    phi = (2.4 * code.double())[:, None] + 0.7 * hh[None, :].double()          # [n,H]
    qt = torch.zeros(n, H, D, dtype=F64)
    kt = torch.zeros(n, H, D, dtype=F64)
    qt[:, :, 0] = g
    kt[:, :, 0] = torch.where(hot[:, None], torch.tensor(g, dtype=F64), g / 4 * phi.cos())
    kt[:, :, half] = torch.where(hot[:, None], torch.zeros((), dtype=F64), g / 4 * phi.sin())
    i = torch.arange(1, half)
    qt[:, :, 1:half] = 0.5
    qt[:, :, half + 1:rot] = 0.5
    kt[:, :, 1:half] = 0.5 * ((i + 1).double() * phi[:, :, None]).cos()
    kt[:, :, half + 1:rot] = 0.5 * ((i + 1).double() * phi[:, :, None]).sin()
    qt[:, :, rot] = 8.0
    kt[:, :, rot] = (base * math.sqrt(D) / 8.0)[:, None]
    dd = torch.arange(rot + 1, D)
    qt[:, :, rot + 1:] = 0.25 * (1 - 2 * (dd % 2)).double()
    kt[:, :, rot + 1:] = 0.125 * (((code[:, None, None] * 7 + dd[None, None, :] * 3 + hh[None, :, None]) % 5) - 2).double()
    rows[:, :, 1] = _rotate(kt, pos, cos, sin, inverse=True)
    if fam != "census":
        rows[:, :, 0] = _rotate(qt, pos, cos, sin, inverse=True)
    return rows


# ------------------------------------------------------------------------------------------------------------------------------
# cases: (kernel, dtype, shape) and what they reach
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    op: str                 # decode | beam | suffix | cand
    dtype: str              # f32 | bf16
    D: int
    H: int
    pads: Tuple[int, ...]   # left padding of every prompt (T: an all-padding prompt); len = B
    P: int = 0              # image keys
    T: int = 0              # text positions of the prompt
    cap: int = 1            # decode / beam: rows of the generated cache
    t: int = 0              # decode / beam: the step
    rot: int = 0            # 0: D // 4
    prerot: bool = False
    flat: bool = True       # decode, pre-rotated: variant 741 (True) or 740
    k: int = 1              # beam
    index: Tuple[int, ...] = ()   # suffix: image_index; N = max + 2 (one image more than used)
    C: int = 1              # cand
    A: int = 1              # cand
    note: str = ""

    @property
    def B(self):
        return len(self.pads)

    @property
    def rotary(self):
        return self.rot or self.D // 4

    @property
    def S0(self):
        return self.P + self.T

    @property
    def path(self) -> str:
        if self.op == "decode":
            return decode_path(self.dtype, self.D, self.rotary, self.S0 + self.t + 1, self.T, self.prerot, self.flat)
        if self.op == "beam":
            return "beam"
        return rows_path(self.dtype, self.D, self.rotary)

    @property
    def id(self) -> str:
        s = f"{self.op}-{self.dtype}-D{self.D}r{self.rotary}-B{self.B}H{self.H}-P{self.P}T{self.T}"
        if self.op == "decode":
            s += f"-t{self.t}c{self.cap}" + (f"-prerot{741 if self.flat else 740}" if self.prerot else "")
        if self.op == "beam":
            s += f"-k{self.k}t{self.t}c{self.cap}"
        if self.op == "cand":
            s += f"-C{self.C}A{self.A}"
        return s

    @property
    def shape(self) -> str:
        return self.id.split("-", 2)[2]


def _both(**kw) -> List[Case]:
    return [Case(dtype=dt, **kw) for dt in ("f32", "bf16")]


def _prerot(**kw) -> List[Case]:
    """fp32 has one kernel for the pre-rotated cache; bf16 runs under variant 740 (online form) and 741 (all rows in flight)"""
    return [Case(dtype="f32", prerot=True, **kw), Case(dtype="bf16", prerot=True, flat=False, **kw), Case(dtype="bf16", prerot=True, flat=True, **kw)]


def decode_cases() -> List[Case]:
    c: List[Case] = []
    # rotation on load.  rot % 16 != 0 or D = 80: the scalar kernel (79 keys: a lane takes two)
    c += _both(op="decode", D=64, rot=20, H=2, pads=(0, 3), P=9, T=5, cap=4, t=2)
    c += _both(op="decode", D=80, rot=20, H=1, pads=(0, 4), P=70, T=7, cap=3, t=1)
    # fused: D = 64 (32 row groups x UNR 5), 128 (16 x 4), 256 (8 x 4); an all-padding prompt
    c += _both(op="decode", D=64, H=2, pads=(0, 4, 13), P=40, T=13, cap=5, t=4)
    c += _both(op="decode", D=128, H=1, pads=(0, 2), P=8, T=6, cap=3, t=2)
    c += _both(op="decode", D=256, H=1, pads=(0, 1), P=5, T=3, cap=2, t=1)
    c += _both(op="decode", D=64, H=2, pads=(0, 1), P=5, T=3, cap=3, t=0, note="nk < groups")
    c += _both(op="decode", D=64, H=1, pads=(0, 7), P=3, T=40, cap=2, t=1, note="P < groups, padded: groups 3..9 start on a masked row")
    c += _both(op="decode", D=64, H=1, pads=(0, 5), P=150, T=8, cap=3, t=2, note="nk = 161: one step of UNR * groups and a row")
    c += _both(op="decode", D=64, H=1, pads=(0, 5), P=310, T=8, cap=3, t=2, note="nk = 321: two steps and a row")
    # pre-rotated cache: both sides of flat <-> fused
    c += _prerot(op="decode", D=64, H=2, pads=(0, 6), P=8, T=6, cap=4, t=0)
    c += _prerot(op="decode", D=256, H=1, pads=(0, 1), P=5, T=3, cap=2, t=1)
    c += _prerot(op="decode", D=64, H=2, pads=(0, 9), P=740, T=20, cap=8, t=7, note="nk = 768, t = cap - 1")
    c += _prerot(op="decode", D=64, H=2, pads=(0, 9), P=748, T=20, cap=4, t=0, note="nk = 769, t = 0")
    c += _prerot(op="decode", D=128, H=1, pads=(0, 4), P=370, T=10, cap=4, t=3, note="nk = 384, t = cap - 1")
    c += _prerot(op="decode", D=128, H=1, pads=(0, 4), P=374, T=10, cap=4, t=0, note="nk = 385, t = 0")
    c += _prerot(op="decode", D=64, H=1, pads=(0, 100), P=4, T=256, cap=2, t=1, note="Tm = 256")
    c += _prerot(op="decode", D=64, H=1, pads=(0, 100), P=4, T=257, cap=2, t=1, note="Tm = 257")
    return c


def beam_cases() -> List[Case]:
    c: List[Case] = []
    # every (k, t) at D = 64; at D = 128 / 256 every k and every t, two t per k
    for di, D in enumerate((64, 128, 256)):
        for ki, k in enumerate((1, 2, 3, 4, 5, 8)):
            for ti, t in enumerate((0, 1, 3)):
                if D == 64 or ti != (ki + di) % 3:
                    c += _both(op="beam", D=D, H=2 if D == 64 else 1, pads=(0, 2), P=6, T=5, cap=4, t=t, k=k, prerot=True)
    return c


def suffix_cases() -> List[Case]:
    c: List[Case] = []
    for P, T in ((64, 1), (63, 1), (1, 63), (63, 64), (64, 65)):     # P + T = 65, 64, 64, 127, 129
        c += _both(op="suffix", D=64, H=2, pads=(0, min(3, T - 1), T), P=P, T=T, index=(2, 0, 2))
    c.append(Case(op="suffix", dtype="bf16", D=128, H=1, pads=(0, 3, 65), P=64, T=65, index=(2, 0, 2)))
    c.append(Case(op="suffix", dtype="bf16", D=256, H=1, pads=(0, 1, 3), P=5, T=3, index=(2, 0, 2)))
    c.append(Case(op="suffix", dtype="bf16", D=80, H=1, pads=(0, 2, 7), P=60, T=7, index=(2, 0, 2), note="bf16 without an MFMA kernel"))
    return c


def cand_cases() -> List[Case]:
    c: List[Case] = []
    c += _both(op="cand", D=64, H=2, pads=(0, 3), P=56, T=8, C=3, A=1, note="S0 = 64")
    c += _both(op="cand", D=64, H=2, pads=(0, 3), P=55, T=8, C=3, A=63, note="C * A = 189 over three query tiles")
    c += _both(op="cand", D=64, H=1, pads=(0, 3), P=57, T=8, C=2, A=64, note="S0 = 65")
    c += _both(op="cand", D=64, H=1, pads=(0, 0), P=64, T=0, C=2, A=65, note="T = 0, no mask, S0 = 64")
    c.append(Case(op="cand", dtype="bf16", D=128, H=1, pads=(0, 2), P=60, T=4, C=2, A=33))
    c.append(Case(op="cand", dtype="bf16", D=80, H=1, pads=(0, 2), P=16, T=4, C=2, A=5, note="bf16 without an MFMA kernel"))
    return c


def all_cases() -> List[Case]:
    return decode_cases() + beam_cases() + suffix_cases() + cand_cases()


# ------------------------------------------------------------------------------------------------------------------------------
# inputs of a (case, family, hot key)
# ------------------------------------------------------------------------------------------------------------------------------
def beam_anc(B: int, k: int, cap: int) -> torch.Tensor:
    """Beams 0 and 1 of a sample share the ancestor slot 1, so beam 0's whole history lives in another slot; beam r >= 2 reads row j
    from slot (r + j + 1) mod k."""
    anc = torch.zeros(B * k, cap, dtype=torch.int32)
    for b in range(B):
        for r in range(k):
            for j in range(cap):
                anc[b * k + r, j] = b * k + (min(1, k - 1) if r < 2 else (r + j + 1) % k)
    return anc


def hot_keys(case: Case) -> List[Tuple]:
    """peaked: where the hot key sits, in turn.  ("key", j): key j of the axis [prefix | generated rows of the sample / text];
    ("slot", r, j): row j of beam slot r of every sample; ("cand", c, i): row i of candidate c of every prompt."""
    P, S0, D = case.P, case.S0, case.D
    chunks = D // 8
    groups = 256 // chunks
    if case.op in ("decode", "beam"):
        n = S0 + case.t + 1
        edges = [0, P - 1, P, S0 - 1, S0, S0 + case.t]
        if case.op == "decode":
            if case.path == "scalar":
                step = [64]                                                             # a lane's second key
            elif case.path == "flat":
                step = [groups, 2 * groups, 10 * groups, 12 * groups, 16 * groups]      # row groups; the UNR 10 / 12 / 16 edges
            else:
                unr = (10 if D == 64 else 8) if case.prerot else (5 if D == 64 else 4)
                step = [groups, unr * groups, 2 * unr * groups]                         # row groups; steps of UNR * groups
        else:
            step = [groups, 4 * groups]                                                 # the beam kernel's prefix step
        edges += [e + o for e in step for o in (-1, 0)]
        keys = sorted({j for j in edges if 0 <= j < n})
        if case.op == "decode":
            return [("key", j) for j in keys]
        out = [("key", j) for j in keys if j < S0]
        slots = sorted({0, min(1, case.k - 1), case.k - 1})
        return out + [("slot", r, j) for j in sorted({0, max(0, case.t - 1), case.t}) for r in slots]
    if case.op == "suffix":
        n = P + case.T
        return [("key", j) for j in sorted({j for j in (0, P - 1, P, n - 1, 63, 64, 127, 128) if 0 <= j < n})]
    CA = case.C * case.A
    pre = sorted({j for j in (0, P - 1, P, S0 - 1, 63, 64) if 0 <= j < S0})
    flat = sorted({r for r in (0, case.A - 1, case.A, 63, 64, 127, 128, CA - 1) if 0 <= r < CA})
    return [("key", j) for j in pre] + [("cand", r // case.A, r % case.A) for r in flat]


def variants(case: Case, fam: str) -> List[Optional[Tuple]]:
    return hot_keys(case) if fam == "peaked" else [None]


def _resolve_hot(case: Case, b: int, j: int) -> int:
    """a hot text key that prompt b pads moves to the prompt's first visible text key, or to the first key behind the text"""
    pad = case.pads[b]
    if case.P <= j < case.S0 and j - case.P < pad:
        return case.P + pad if pad < case.T else (case.S0 if case.op != "suffix" else case.P - 1)
    return j


def build(case: Case, fam: str, hot: Optional[Tuple] = None) -> Dict[str, torch.Tensor]:
    """The tensors the kernel reads, as fp64 values that the case's dtype holds exactly, and the rotary tables."""
    B, H, D, P, T, S0, rot = case.B, case.H, case.D, case.P, case.T, case.S0, case.rotary
    n_pos = {"decode": S0 + case.cap, "beam": S0 + case.cap, "suffix": S0, "cand": S0 + case.A}[case.op] + 2
    cos, sin = tables(D, rot, n_pos)
    am = torch.ones(B, T, dtype=torch.int64)
    for b in range(B):
        am[b, : case.pads[b]] = 0
    total = {"decode": S0 + case.t + 1, "beam": S0 + case.t + 1, "suffix": S0, "cand": S0 + case.A}[case.op]
    ramp = lambda pos: torch.as_tensor(pos, dtype=F64) / max(1, total - 1)

    def mk(pos, hot_mask, masked, code):
        pos = torch.as_tensor(pos)
        return rnd(make_rows(fam, H, D, rot, pos, ramp(pos), hot_mask, masked, code, cos, sin), case.dtype)

    def hot_key(b):
        return _resolve_hot(case, b, hot[1]) if hot is not None and hot[0] == "key" else -1

    out: Dict[str, torch.Tensor] = {"cos": cos, "sin": sin, "am": am}
    if case.op == "suffix":
        N = max(case.index) + 2
        jj = torch.arange(P)
        # the image store is shared: the hot image key is hot for every prompt of that image
        out["qkv_img"] = torch.stack([mk(jj, jj == hot_key(0), torch.zeros(P, dtype=torch.bool), jj + 301 * n) for n in range(N)])
        tt = P + torch.arange(T)
        out["qkv_txt"] = torch.stack([mk(tt, tt == hot_key(b), am[b] == 0, tt + 101 * b) for b in range(B)])
        out["index"] = torch.tensor(case.index, dtype=torch.int64)
        return out
    jj = torch.arange(S0)
    pre = torch.stack([mk(jj, jj == hot_key(b), _pad_keys(am[b], P, S0, S0), jj + 101 * b) for b in range(B)])
    if case.op == "cand":
        ii = S0 + torch.arange(case.A)
        out["qkv_pre"] = pre
        out["qkv_cand"] = torch.stack([torch.stack([
            mk(ii, (ii - S0 == hot[2]) if hot is not None and hot[0] == "cand" and hot[1] == c else torch.zeros(case.A, dtype=torch.bool),
               torch.zeros(case.A, dtype=torch.bool), ii + 101 * b + 211 * (c + 1)) for c in range(case.C)]) for b in range(B)])
        return out
    # decode / beam: raw rows first, then the cache as the loop leaves it before step t
    slots = B * case.k if case.op == "beam" else B
    ii = S0 + torch.arange(case.cap)
    new = []
    for r in range(slots):
        b, local = (r // case.k, r % case.k) if case.op == "beam" else (r, 0)
        if hot is not None and hot[0] == "slot":
            hm = (ii - S0 == hot[2]) if local == hot[1] else torch.zeros(case.cap, dtype=torch.bool)
        else:
            hm = ii == hot_key(b)     # beam: the hot prefix keys lie before S0
        new.append(mk(ii, hm, torch.zeros(case.cap, dtype=torch.bool), ii + 101 * b + 211 * (local + 1)))
    new = torch.stack(new)
    new[:, case.t + 1:] = 0.0     # rows behind the step are not written yet
    if case.prerot:
        pre = rnd(rotate_k(pre, S0, H, D, rot, cos, sin), case.dtype)
        new_rot = rnd(rotate_k(new, case.cap, H, D, rot, cos[S0:], sin[S0:]), case.dtype)
        new[:, : case.t] = new_rot[:, : case.t]
    out["prefix"], out["new"] = pre, new
    if case.op == "beam":
        out["anc"] = beam_anc(B, case.k, case.cap)
    return out


def groups_of(case: Case, inp: Dict[str, torch.Tensor]) -> List[Group]:
    if case.op == "decode":
        return decode_groups(inp["prefix"], inp["new"], case.t, inp["am"], case.P, case.prerot)
    if case.op == "beam":
        return decode_beam_groups(inp["prefix"], inp["new"], inp["anc"], case.t, case.k, inp["am"], case.P)
    if case.op == "suffix":
        return suffix_groups(inp["qkv_img"], inp["index"], inp["qkv_txt"], inp["am"])
    return cand_groups(inp["qkv_pre"], inp["qkv_cand"], inp["am"] if case.T else None)


def reference(case: Case, inp: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    rot, cos, sin = case.rotary, inp["cos"], inp["sin"]
    if case.op == "decode":
        return decode(inp["prefix"], inp["new"], case.t, inp["am"], case.P, rot, cos, sin, case.prerot)
    if case.op == "beam":
        return decode_beam(inp["prefix"], inp["new"], inp["anc"], case.t, case.k, inp["am"], case.P, rot, cos, sin)
    if case.op == "suffix":
        return suffix(inp["qkv_img"], inp["index"], inp["qkv_txt"], inp["am"], rot, cos, sin)
    return cand(inp["qkv_pre"], inp["qkv_cand"], inp["am"] if case.T else None, rot, cos, sin)
