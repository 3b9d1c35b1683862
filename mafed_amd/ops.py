"""Thin tensor-level wrappers over the C-ABI (one Python function per entry point of include/mafed_hip.h).

Every wrapper launches on torch's current HIP stream and never synchronises.  Tensors must live on the GPU;
there is deliberately no CPU implementation behind these names.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from mafed_amd import _lib
import contextlib
import ctypes as C
import threading

from mafed_amd._lib import BF16, EPI_GELU, EPI_GELU_BWD, EPI_NO_PERSISTENT, EPI_NONE, EPI_QUICK_GELU, EPI_RES1_BF16, EPI_TICKETED, F32, check  # noqa: F401


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _ptr(t: Optional[torch.Tensor]) -> int:
    if t is None:
        return 0
    if not t.is_cuda:
        raise _lib.MafedHipError("mafed_amd ops need GPU tensors (no CPU fallback)")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """Raw handle of the caller's current HIP stream.  Through the two C entry points directly when this torch has them:
    ``torch.cuda.current_stream()`` builds a Stream object and resolves the device index through ``is_available()`` on every call
    (3 of the 15 ms the host spent enqueueing a 410M MAFED step, ~650 launches)."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


class _Fn:
    """Lazily bound entry points (one attribute lookup per call instead of load() + getattr)."""

    def __getattr__(self, name):
        fn = getattr(_lib.load(), "mafed_" + name)
        setattr(self, name, fn)
        return fn


_fn = _Fn()


class Workspace:
    """Grow-only scratch buffer handed to kernels that need one (no allocation inside the library)."""

    def __init__(self, device):
        self.device = device
        self.buf = torch.empty(1 << 20, dtype=torch.uint8, device=device)

    def get(self, nbytes: int) -> torch.Tensor:
        if self.buf.numel() < nbytes:
            self.buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
        return self.buf


_workspaces = {}


def workspace(device) -> Workspace:
    key = (device.type, device.index)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = Workspace(device)
    return ws


_tls = threading.local()


@contextlib.contextmanager
def no_persistent_gemm(on: bool = True):
    """Inside this block the CALLING THREAD's ``gemm`` / ``gemm_grouped`` calls carry MAFED_EPI_NO_PERSISTENT: each of those launches keeps
    off the one-block-per-CU persistent kernels (e.g. a backward that runs beside collectives).  A per-call flag in the C-ABI, a
    thread-local here: nothing process-wide is touched, other threads / models / forced tuning variants are unaffected."""
    prev = getattr(_tls, "no_pp", 0)
    _tls.no_pp = EPI_NO_PERSISTENT if on else prev
    try:
        yield
    finally:
        _tls.no_pp = prev


@contextlib.contextmanager
def ticketed_gemm(on: bool = True):
    """Inside this block the calling thread's ``gemm`` / ``gemm_grouped`` calls carry MAFED_EPI_TICKETED: a launch that takes a persistent
    kernel over several rounds draws its tiles from per-XCD queues (a backward that runs beside collectives or other long-resident
    kernels).  Per call in the C-ABI, thread-local here, like :func:`no_persistent_gemm`."""
    prev = getattr(_tls, "no_pp", 0)
    _tls.no_pp = (prev | EPI_TICKETED) if on else prev
    try:
        yield
    finally:
        _tls.no_pp = prev


def gemm(A: torch.Tensor, B: torch.Tensor, transA: bool, transB: bool, out: Optional[torch.Tensor] = None,
         out_dtype: Optional[torch.dtype] = None, bias: Optional[torch.Tensor] = None, epilogue: int = EPI_NONE,
         aux: Optional[torch.Tensor] = None, res1: Optional[torch.Tensor] = None, res2: Optional[torch.Tensor] = None,
         beta: float = 0.0, colsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = op(A) @ op(B) with the fused epilogue of mafed_gemm.  A, B 2-D, same dtype (bf16 -> MFMA, f32 -> exact).
    ``colsum`` (fp32 [N]): += the column sums of the stored C (mafed_gemm_colsum)."""
    assert A.dim() == 2 and B.dim() == 2 and A.dtype == B.dtype
    assert A.stride(1) == 1 and B.stride(1) == 1
    M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    N = B.shape[0] if transB else B.shape[1]
    Kb = B.shape[1] if transB else B.shape[0]
    assert K == Kb, (A.shape, B.shape, transA, transB)
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or A.dtype, device=A.device)
    assert out.shape == (M, N) and out.stride(1) == 1
    if res1 is not None and res1.dtype == torch.bfloat16:
        epilogue |= EPI_RES1_BF16
    epilogue |= getattr(_tls, "no_pp", 0)
    if colsum is None:
        rc = _fn.gemm(_dt(A), int(transA), int(transB), M, N, K, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out),
                      out.stride(0), _dt(out), _ptr(bias), epilogue, _ptr(aux), _ptr(res1), _ptr(res2), float(beta), _stream())
    else:
        assert colsum.dtype == torch.float32 and colsum.numel() == N and colsum.is_contiguous()
        rc = _fn.gemm_colsum(_dt(A), int(transA), int(transB), M, N, K, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out),
                             out.stride(0), _dt(out), _ptr(bias), epilogue, _ptr(aux), _ptr(res1), _ptr(res2), float(beta),
                             _ptr(colsum), _stream())
    if rc:
        check(rc, "mafed_gemm")
    return out


def gemm_grouped(problems, transA: bool, transB: bool) -> None:
    """Several independent ``C_i = op(A_i) @ op(B_i)`` as one persistent launch (mafed_gemm_grouped).  ``problems``: dicts with the
    keyword arguments of :func:`gemm` (``A``, ``B``, ``out`` required; ``bias``, ``epilogue``, ``aux``, ``res1``, ``res2``, ``beta``,
    ``colsum`` optional; ``sumsq`` = 16 fp32 slots that receive += the squares of the stored fp32 C).  All share the operand layouts, the input dtype and the output dtype."""
    n = len(problems)
    if n == 0:
        return
    arr = (_lib.GemmProblem * n)()
    in_dt = out_dt = None
    for i, q in enumerate(problems):
        A, B, out = q["A"], q["B"], q["out"]
        assert A.dim() == 2 and B.dim() == 2 and A.dtype == B.dtype and A.stride(1) == 1 and B.stride(1) == 1 and out.stride(1) == 1
        M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
        N = B.shape[0] if transB else B.shape[1]
        assert K == (B.shape[1] if transB else B.shape[0]) and out.shape == (M, N)
        in_dt = _dt(A) if in_dt is None else in_dt
        out_dt = _dt(out) if out_dt is None else out_dt
        assert _dt(A) == in_dt and _dt(out) == out_dt, "a grouped launch shares its input and output types"
        epi = q.get("epilogue", EPI_NONE) | getattr(_tls, "no_pp", 0)
        res1 = q.get("res1")
        if res1 is not None and res1.dtype == torch.bfloat16:
            epi |= EPI_RES1_BF16
        cs = q.get("colsum")
        assert cs is None or (cs.dtype == torch.float32 and cs.numel() == N and cs.is_contiguous())
        g = arr[i]
        g.M, g.N, g.K = M, N, K
        g.A, g.lda, g.B, g.ldb, g.C, g.ldc = _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out), out.stride(0)
        g.bias, g.epilogue, g.aux = _ptr(q.get("bias")), epi, _ptr(q.get("aux"))
        g.res1, g.res2, g.beta, g.colsum = _ptr(res1), _ptr(q.get("res2")), float(q.get("beta", 0.0)), _ptr(cs)
        sq = q.get("sumsq")
        assert sq is None or (sq.dtype == torch.float32 and sq.numel() >= 16 and sq.is_contiguous() and out.dtype == torch.float32)
        g.sumsq = _ptr(sq)
    rc = _fn.gemm_grouped(in_dt, int(transA), int(transB), out_dt, arr, n, _stream())
    if rc:
        check(rc, "mafed_gemm_grouped")


def colsum_(X: torch.Tensor, out: torch.Tensor) -> None:
    """out[n] += sum_m X[m, n]"""
    assert X.dim() == 2 and X.stride(1) == 1 and out.dtype == torch.float32
    M, N = X.shape
    check(_lib.load().mafed_colsum(_ptr(X), _dt(X), M, N, X.stride(0), _ptr(out), 0, 0, _stream()), "mafed_colsum")


def layernorm_fwd(x: torch.Tensor, w1, b1, w2=None, b2=None, eps: float = 1e-5, out_dtype=torch.float32, save_stats: bool = True):
    rows, h = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    y1 = torch.empty((rows, h), dtype=out_dtype, device=x.device)
    y2 = torch.empty_like(y1) if w2 is not None else None
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    check(_lib.load().mafed_layernorm_fwd(_ptr(x), rows, h, eps, _ptr(w1), _ptr(b1), _ptr(y1), _ptr(w2), _ptr(b2), _ptr(y2),
                                          _dt(y1), _ptr(mean), _ptr(rstd), _stream()), "mafed_layernorm_fwd")
    return y1, y2, mean, rstd


class TeacherRows:
    """The frozen teacher's hidden state of ONE layer for the samples of a batch, not materialised: ``states`` is that layer's slab of a
    resident teacher cache, [n, S, h] fp32 or bf16, and ``index`` [B] int32 names the batch's samples within it (None: the states ARE
    the batch, [B, S, h] -- a dense teacher that is not fp32).  The distillation
    kernels (``distill_fwd / bwd``, ``distill_cls_fwd / bwd``, the injection of ``layernorm_bwd`` / ``layernorm_bwd_rows``) take it
    wherever they take a dense fp32 [B, S, h] teacher tensor and read row ``index[b] * S + s`` in place, widening bf16 at the load.
    Anything else calls ``materialize()``."""
    __slots__ = ("states", "index")

    def __init__(self, states: torch.Tensor, index: Optional[torch.Tensor] = None):
        if states.dim() != 3 or states.dtype not in (torch.float32, torch.bfloat16) or not states.is_contiguous():
            raise ValueError("TeacherRows: states must be a contiguous [n, S, h] fp32 / bf16 tensor")
        if index is not None and (index.dim() != 1 or index.dtype != torch.int32 or not index.is_contiguous() or index.device != states.device):
            raise ValueError("TeacherRows: index must be a contiguous int32 [B] tensor on the device of the states")
        self.states, self.index = states, index

    @property
    def shape(self):
        return (self.states.shape[0] if self.index is None else self.index.numel(), self.states.shape[1], self.states.shape[2])

    @property
    def dtype(self):
        return self.states.dtype

    def record_stream(self, stream) -> None:
        self.states.record_stream(stream)
        if self.index is not None:
            self.index.record_stream(stream)

    def materialize(self) -> torch.Tensor:
        """The dense fp32 [B, S, h] tensor these rows stand for (``gather_rows`` + an exact upcast of bf16 rows)."""
        n, S, h = self.states.shape
        if self.index is None:
            return self.states if self.states.dtype == torch.float32 else cast(self.states, torch.float32)
        if n * S >= 2 ** 31:
            raise RuntimeError(f"TeacherRows.materialize: {n} samples x {S} tokens exceed the 32-bit row ids of the gather kernel")
        B = self.index.numel()
        rows = (self.index.view(B, 1) * S + torch.arange(S, device=self.index.device, dtype=torch.int32).view(1, S)).view(-1)
        out = gather_rows(self.states.view(n * S, h), rows)
        return (out if out.dtype == torch.float32 else cast(out, torch.float32)).view(B, S, h)


def _teacher(t, B: Optional[int] = None, S: Optional[int] = None, h: Optional[int] = None):
    """(pointer, mafed_dtype, index pointer) of a teacher argument: a dense fp32 tensor (no index), ``TeacherRows``, or None."""
    if t is None:
        return 0, F32, 0
    if isinstance(t, TeacherRows):
        if (B is not None and t.shape[0] != B) or (S is not None and t.shape[1] != S) or (h is not None and t.shape[2] != h):
            raise ValueError(f"TeacherRows of shape {t.shape} for a batch of [{B}, {S}, {h}]")
        return _ptr(t.states), _dt(t.states), _ptr(t.index)
    assert t.dtype == torch.float32 and t.is_contiguous()
    return _ptr(t), F32, 0


def layernorm_bwd(dy1, dy2, x, mean, rstd, w1, w2, dres, dw1, db1, dw2=None, db2=None, want_lp: bool = False,
                  teacher=None, attention_mask=None, S: int = 0, P: int = 0, inj_scale=None, inj_mul: float = 1.0,
                  dxsum_a=None, dxsum_b=None):
    rows, h = x.shape
    dx = torch.empty((rows, h), dtype=torch.float32, device=x.device)
    dx_lp = torch.empty((rows, h), dtype=dy1.dtype, device=x.device) if want_lp else None
    lib = _lib.load()
    nb = lib.mafed_layernorm_bwd_workspace_bytes(rows, h)
    ws = workspace(x.device).get(nb)
    tp, tdt, tix = _teacher(teacher, rows // S if S else None, S or None, h)
    check(lib.mafed_layernorm_bwd_indexed(_ptr(dy1), _ptr(dy2), _dt(dy1), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(w1), _ptr(w2), rows, h,
                                          _ptr(dres), _ptr(dx), _ptr(dx_lp), _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), tp, tdt, tix,
                                          _ptr(attention_mask), S, P, S - P, _ptr(inj_scale), float(inj_mul), _ptr(dxsum_a), _ptr(dxsum_b), _ptr(ws),
                                          ws.numel(), _stream()),
          "mafed_layernorm_bwd")
    return dx, dx_lp


def layernorm_bwd_rows(dy1, dy2, x, mean, rstd, w1, w2, dres, want_lp: bool = False, teacher=None, attention_mask=None, S: int = 0, P: int = 0,
                       inj_scale=None, inj_mul: float = 1.0, want_dxsum: bool = False):
    """Row kernel of the LayerNorm backward alone -> (dx, dx_lp, partials); ``partials`` is a private buffer that
    ``layernorm_bwd_params`` folds into the parameter gradients later (on another stream, ordered by the caller)."""
    rows, h = x.shape
    dx = torch.empty((rows, h), dtype=torch.float32, device=x.device)
    dx_lp = torch.empty((rows, h), dtype=dy1.dtype, device=x.device) if want_lp else None
    lib = _lib.load()
    ws = torch.empty(lib.mafed_layernorm_bwd_workspace_bytes(rows, h), dtype=torch.uint8, device=x.device)
    tp, tdt, tix = _teacher(teacher, rows // S if S else None, S or None, h)
    check(lib.mafed_layernorm_bwd_rows_indexed(_ptr(dy1), _ptr(dy2), _dt(dy1), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(w1), _ptr(w2), rows, h,
                                               _ptr(dres), _ptr(dx), _ptr(dx_lp), tp, tdt, tix, _ptr(attention_mask), S, P, S - P, _ptr(inj_scale),
                                               float(inj_mul), 1 if want_dxsum else 0, _ptr(ws), ws.numel(), _stream()), "mafed_layernorm_bwd_rows")
    return dx, dx_lp, ws


def layernorm_bwd_params(ws: torch.Tensor, rows: int, h: int, dw1, db1, dw2=None, db2=None, dxsum_a=None, dxsum_b=None) -> None:
    check(_lib.load().mafed_layernorm_bwd_params(rows, h, _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(dxsum_a), _ptr(dxsum_b), _ptr(ws),
                                                 ws.numel(), _stream()), "mafed_layernorm_bwd_params")


def attn_fwd(qkv: torch.Tensor, B: int, S: int, H: int, D: int, rot: int, cos, sin, attention_mask: torch.Tensor):
    T = attention_mask.shape[1]
    out = torch.empty((B * S, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
    check(_lib.load().mafed_attn_fwd(_ptr(qkv), _dt(qkv), B, S, H, D, rot, _ptr(cos), _ptr(sin), _ptr(attention_mask), T, _ptr(out),
                                     _ptr(lse), _stream()), "mafed_attn_fwd")
    return out, lse


def attn_fwd_exact_bf16(qkv, B, S, H, D, rot, cos, sin, attention_mask):
    T = attention_mask.shape[1]
    out = torch.empty((B * S, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
    check(_lib.load().mafed_attn_fwd_exact_bf16(_ptr(qkv), B, S, H, D, rot, _ptr(cos), _ptr(sin), _ptr(attention_mask), T, _ptr(out),
                                                _ptr(lse), _stream()), "mafed_attn_fwd_exact_bf16")
    return out, lse


def attn_bwd(qkv, out, dout, lse, B, S, H, D, rot, cos, sin, attention_mask, colsum: Optional[torch.Tensor] = None):
    """dqkv; ``colsum`` (fp32 [3*H*D]) += the column sums of dqkv (query_key_value.bias gradient, mafed_attn_bwd_colsum)."""
    T = attention_mask.shape[1]
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
    if colsum is None:
        check(_lib.load().mafed_attn_bwd(_ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _dt(qkv), B, S, H, D, rot, _ptr(cos), _ptr(sin),
                                         _ptr(attention_mask), T, _ptr(dqkv), _ptr(delta), _stream()), "mafed_attn_bwd")
    else:
        assert colsum.dtype == torch.float32 and colsum.numel() == 3 * H * D and colsum.is_contiguous()
        check(_lib.load().mafed_attn_bwd_colsum(_ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _dt(qkv), B, S, H, D, rot, _ptr(cos),
                                                _ptr(sin), _ptr(attention_mask), T, _ptr(dqkv), _ptr(delta), _ptr(colsum), _stream()),
              "mafed_attn_bwd_colsum")
    return dqkv


def attn_fwd_bidir(qkv: torch.Tensor, B: int, S: int, H: int, D: int, out: Optional[torch.Tensor] = None):
    """Bidirectional attention of the CLIP vision tower: qkv [>= B*S, H*3*D] -> out [>= B*S, H*D] (rows past B*S untouched)."""
    assert qkv.dim() == 2 and qkv.shape[1] == 3 * H * D and qkv.shape[0] >= B * S and qkv.is_contiguous()
    if out is None:
        out = torch.empty((B * S, H * D), dtype=qkv.dtype, device=qkv.device)
    assert out.dtype == qkv.dtype and out.shape[0] >= B * S and out.shape[1] == H * D and out.is_contiguous()
    lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
    check(_lib.load().mafed_attn_fwd_bidir(_ptr(qkv), _dt(qkv), B, S, H, D, _ptr(out), _ptr(lse), _stream()), "mafed_attn_fwd_bidir")
    return out


def patchify(pixels: torch.Tensor, patch: int, rows_out: int, k_pad: int, out_dtype: torch.dtype) -> torch.Tensor:
    """im2col of the patch convolution: pixels [B,C,H,W] -> [rows_out, k_pad] (zero padding rows / columns)."""
    B, C, H, W = pixels.shape
    assert pixels.is_contiguous()
    out = torch.empty((rows_out, k_pad), dtype=out_dtype, device=pixels.device)
    check(_lib.load().mafed_patchify(_ptr(pixels), _dt(pixels), B, C, H, W, int(patch), int(rows_out), int(k_pad), _ptr(out), _dt(out), _stream()),
          "mafed_patchify")
    return out


def vit_assemble(patch_emb: torch.Tensor, class_embedding: torch.Tensor, position_embedding: torch.Tensor, B: int, num_patches: int, h: int,
                 out: torch.Tensor) -> torch.Tensor:
    """out[b, 0] = cls + pos[0]; out[b, 1 + p] = patch_emb[b * np + p] + pos[1 + p]   (fp32 rows of ``out`` [>= B*(np+1), h])"""
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] >= B * (num_patches + 1) and out.shape[1] == h
    assert class_embedding.dtype == torch.float32 and position_embedding.dtype == torch.float32 and position_embedding.is_contiguous()
    check(_lib.load().mafed_vit_assemble(_ptr(patch_emb), _dt(patch_emb), patch_emb.stride(0), _ptr(class_embedding), _ptr(position_embedding), B,
                                         num_patches, h, _ptr(out), _stream()), "mafed_vit_assemble")
    return out


def rotate_k_rows_(qkv: torch.Tensor, B: int, S: int, H: int, D: int, rot: int, cos, sin) -> None:
    """k part of a [B*S, H*3*D] (or [B,S,...]) qkv tensor rotated in place for each row's position (mafed_rotate_k_rows)."""
    assert qkv.is_contiguous() and qkv.numel() == B * S * H * 3 * D and cos.shape[0] >= S
    check(_lib.load().mafed_rotate_k_rows(_ptr(qkv), _dt(qkv), B, S, H, D, rot, _ptr(cos), _ptr(sin), _stream()), "mafed_rotate_k_rows")


def attn_decode(qkv_prefix: torch.Tensor, S0: int, qkv_new: torch.Tensor, t: int, B: int, H: int, D: int, rot: int, cos, sin,
                attention_mask: torch.Tensor, prerot: bool = False) -> torch.Tensor:
    """One decode step of attention: query = row t of ``qkv_new`` [B,cap,3*H*D], keys = the prefill's ``qkv_prefix``
    [B*S0, 3*H*D] followed by rows 0..t of ``qkv_new``.  -> [B, H*D]"""
    cap = qkv_new.shape[1]
    assert qkv_new.dim() == 3 and qkv_new.is_contiguous() and qkv_prefix.is_contiguous() and qkv_new.dtype == qkv_prefix.dtype
    assert cos.shape[0] >= S0 + t + 1
    out = torch.empty((B, H * D), dtype=qkv_new.dtype, device=qkv_new.device)
    fn = _lib.load().mafed_attn_decode_prerot if prerot else _lib.load().mafed_attn_decode
    check(fn(_ptr(qkv_prefix), S0, _ptr(qkv_new), cap, t, _dt(qkv_new), B, H, D, rot, _ptr(cos), _ptr(sin),
             _ptr(attention_mask), attention_mask.shape[1], _ptr(out), _stream()), "mafed_attn_decode")
    return out


def attn_decode_beam(qkv_prefix: torch.Tensor, S0: int, qkv_new: torch.Tensor, t: int, B: int, k: int, anc: torch.Tensor, H: int, D: int,
                     rot: int, cos, sin, attention_mask: torch.Tensor) -> torch.Tensor:
    """Decode attention of the k beams of B samples (mafed_attn_decode_beam): queries = row t of every slot of ``qkv_new`` [B*k,cap,3*H*D],
    keys = the sample's pre-rotated prefix ``qkv_prefix`` [B*S0, 3*H*D] (read once for its k beams), then rows j < t of slot
    ``anc[r, j]`` and row t of the beam's own slot.  ``anc`` int32 [B*k, cap].  -> [B*k, H*D]"""
    cap = qkv_new.shape[1]
    assert qkv_new.dim() == 3 and qkv_new.shape[0] == B * k and qkv_new.is_contiguous() and qkv_prefix.is_contiguous()
    assert qkv_new.dtype == qkv_prefix.dtype and anc.dtype == torch.int32 and anc.shape == (B * k, cap) and anc.is_contiguous()
    assert cos.shape[0] >= S0 + t + 1
    out = torch.empty((B * k, H * D), dtype=qkv_new.dtype, device=qkv_new.device)
    check(_lib.load().mafed_attn_decode_beam(_ptr(qkv_prefix), S0, _ptr(qkv_new), cap, t, _dt(qkv_new), B, k, _ptr(anc), H, D, rot, _ptr(cos),
                                             _ptr(sin), _ptr(attention_mask), attention_mask.shape[1], _ptr(out), _stream()), "mafed_attn_decode_beam")
    return out


def _image_index(image_index: Optional[torch.Tensor], N: int, B: int, device) -> Optional[torch.Tensor]:
    if image_index is None:
        assert N == B, f"no image_index: N ({N}) must equal B ({B})"
        return None
    assert image_index.dtype == torch.int64 and image_index.shape == (B,) and image_index.is_contiguous() and image_index.device == device
    return image_index


def attn_suffix_fwd(qkv_img: torch.Tensor, image_index: Optional[torch.Tensor], N: int, P: int, qkv_txt: torch.Tensor, T: int, B: int, H: int,
                    D: int, rot: int, cos, sin, attention_mask: torch.Tensor) -> torch.Tensor:
    """Attention of the T text rows of B prompts over [image image_index[b] | own text] (mafed_attn_suffix_fwd) = rows P .. P+T-1 of
    ``attn_fwd`` on the assembled sequence.  ``qkv_img`` [N*P, 3*H*D], ``qkv_txt`` [B*T, 3*H*D], ``image_index`` int64 [B] on the device
    with values in [0, N) (the caller checks them; None = identity, N == B), ``attention_mask`` [B, T].  -> [B*T, H*D]"""
    assert qkv_img.is_contiguous() and qkv_txt.is_contiguous() and qkv_img.dtype == qkv_txt.dtype
    assert qkv_img.numel() == N * P * 3 * H * D and qkv_txt.numel() == B * T * 3 * H * D
    assert attention_mask.shape == (B, T) and attention_mask.dtype == torch.int64 and attention_mask.is_contiguous()
    assert cos.shape[0] >= P + T
    image_index = _image_index(image_index, N, B, qkv_txt.device)
    out = torch.empty((B * T, H * D), dtype=qkv_txt.dtype, device=qkv_txt.device)
    check(_lib.load().mafed_attn_suffix_fwd(_ptr(qkv_img), _ptr(image_index), N, P, _ptr(qkv_txt), T, _dt(qkv_txt), B, H, D, rot, _ptr(cos),
                                            _ptr(sin), _ptr(attention_mask), _ptr(out), _stream()), "mafed_attn_suffix_fwd")
    return out


def prefix_gather(qkv_img: torch.Tensor, qkv_txt: torch.Tensor, image_index: Optional[torch.Tensor], B: int, P: int, T: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decode cache's prefix of every layer in one launch (mafed_prefix_gather): ``qkv_img`` [L, N*P, W] and ``qkv_txt`` [L, B*T, W]
    -> [L, B*(P+T), W], per prompt the rows of image ``image_index[b]`` followed by its own text rows."""
    L, NP, W = qkv_img.shape
    N = NP // P
    assert NP == N * P and qkv_txt.shape == (L, B * T, W) and qkv_img.dtype == qkv_txt.dtype and qkv_img.is_contiguous() and qkv_txt.is_contiguous()
    image_index = _image_index(image_index, N, B, qkv_txt.device)
    if out is None:
        out = torch.empty((L, B * (P + T), W), dtype=qkv_txt.dtype, device=qkv_txt.device)
    assert out.shape == (L, B * (P + T), W) and out.dtype == qkv_txt.dtype and out.is_contiguous()
    check(_lib.load().mafed_prefix_gather(_ptr(qkv_img), _ptr(qkv_txt), _ptr(image_index), L, N, B, P, T, W, _dt(qkv_txt), _ptr(out), _stream()),
          "mafed_prefix_gather")
    return out


def attn_cand_fwd(qkv_prefix: torch.Tensor, S0: int, qkv_cand: torch.Tensor, C: int, A: int, B: int, H: int, D: int, rot: int, cos, sin,
                  attention_mask: torch.Tensor) -> torch.Tensor:
    """Attention of the A rows of each of the C candidates of B prompts over [prefix b | own earlier rows] (mafed_attn_cand_fwd) = rows
    S0 .. S0+A-1 of ``attn_fwd`` on every assembled [prefix b | candidate (b, c)].  ``qkv_prefix`` [B*S0, 3*H*D] (keys un-rotated),
    ``qkv_cand`` [B*C*A, 3*H*D], ``attention_mask`` [B, T] of the prefix text.  -> [B*C*A, H*D]"""
    assert qkv_prefix.is_contiguous() and qkv_cand.is_contiguous() and qkv_prefix.dtype == qkv_cand.dtype
    assert qkv_prefix.numel() == B * S0 * 3 * H * D and qkv_cand.numel() == B * C * A * 3 * H * D
    assert attention_mask.dim() == 2 and attention_mask.shape[0] == B and attention_mask.dtype == torch.int64 and attention_mask.is_contiguous()
    assert cos.shape[0] >= S0 + A
    out = torch.empty((B * C * A, H * D), dtype=qkv_cand.dtype, device=qkv_cand.device)
    check(_lib.load().mafed_attn_cand_fwd(_ptr(qkv_prefix), S0, _ptr(qkv_cand), C, A, _dt(qkv_cand), B, H, D, rot, _ptr(cos), _ptr(sin),
                                          _ptr(attention_mask), attention_mask.shape[1], _ptr(out), _stream()), "mafed_attn_cand_fwd")
    return out


def token_logprob(logits: torch.Tensor, target: torch.Tensor, logits_row: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``logits[row(r), target[r]] - logsumexp(logits[row(r)])`` in fp32 (mafed_token_logprob).  ``logits`` [N, V] fp32 / bf16 with unit
    column stride (any row stride), ``target`` int64 of any shape (R elements; < 0 gives 0), ``logits_row`` int32 [R] with values in
    [0, N) naming the logits row of every output (None: row r, R <= N).  -> fp32, the shape of ``target``"""
    N, V = logits.shape
    R = target.numel()
    assert logits.stride(1) == 1 and target.dtype == torch.int64 and target.is_contiguous()
    assert (R <= N) if logits_row is None else (logits_row.dtype == torch.int32 and logits_row.numel() == R and logits_row.is_contiguous())
    out = torch.empty(target.shape, dtype=torch.float32, device=logits.device)
    check(_lib.load().mafed_token_logprob(_ptr(logits), _dt(logits), logits.stride(0), _ptr(logits_row), _ptr(target), R, V, _ptr(out), _stream()),
          "mafed_token_logprob")
    return out


def score_reduce(token_logprobs: torch.Tensor, mask: Optional[torch.Tensor], mean: bool) -> torch.Tensor:
    """Per candidate, the sum (``mean``: the mean) of its tokens' log-probabilities over ``mask`` != 0; -inf without a token
    (mafed_score_reduce).  ``token_logprobs`` fp32 [..., A], ``mask`` int64 of the same shape or None.  -> fp32 [...]"""
    A = token_logprobs.shape[-1]
    R = token_logprobs.numel() // A
    assert token_logprobs.dtype == torch.float32 and token_logprobs.is_contiguous()
    assert mask is None or (mask.dtype == torch.int64 and mask.shape == token_logprobs.shape and mask.is_contiguous())
    out = torch.empty(token_logprobs.shape[:-1], dtype=torch.float32, device=token_logprobs.device)
    check(_lib.load().mafed_score_reduce(_ptr(token_logprobs), _ptr(mask), R, A, int(bool(mean)), _ptr(out), _stream()), "mafed_score_reduce")
    return out


def beam_candidates(logits: torch.Tensor, score: torch.Tensor, B: int, k: int, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """Per sample, the top 2k of ``log_softmax(logits[row]) + score[row]`` over its kin = rows / B rows (mafed_beam_candidates).
    logits [B*kin, V] fp32 / bf16 (unit column stride), score fp32 [B*kin] -> (score fp32 [B,2k], token int64 [B,2k], parent int32 [B,2k]),
    best first; equal scores go to the lower flat index row * V + token."""
    rows, V = logits.shape
    assert logits.stride(1) == 1 and rows % B == 0 and score.dtype == torch.float32 and score.numel() == rows and score.is_contiguous()
    dev = logits.device
    if out is None:
        out = (torch.empty((B, 2 * k), dtype=torch.float32, device=dev), torch.empty((B, 2 * k), dtype=torch.int64, device=dev),
               torch.empty((B, 2 * k), dtype=torch.int32, device=dev))
    cs, ct, cp = out
    check(_lib.load().mafed_beam_candidates(_ptr(logits), _dt(logits), logits.stride(0), _ptr(score), B, rows // B, V, k, _ptr(cs), _ptr(ct),
                                            _ptr(cp), _stream()), "mafed_beam_candidates")
    return cs, ct, cp


def beam_update(cand, B: int, k: int, step: int, cap: int, eos: int, pad: int, early_stopping: int, length_penalty: float, run_score,
                anc, hist, fin_tok, fin_score, fin_len, done, next_token) -> None:
    """One step of the beam bookkeeping (mafed_beam_update).  ``anc`` / ``hist`` / ``fin_tok`` / ``fin_score`` / ``fin_len`` are
    (before, after) pairs of distinct tensors; ``run_score``, ``done`` and ``next_token`` are updated in place."""
    cs, ct, cp = cand
    check(_lib.load().mafed_beam_update(_ptr(cs), _ptr(ct), _ptr(cp), B, k, step, cap, int(eos), int(pad), int(early_stopping), float(length_penalty),
                                        _ptr(run_score), _ptr(anc[0]), _ptr(anc[1]), _ptr(hist[0]), _ptr(hist[1]), _ptr(fin_tok[0]), _ptr(fin_tok[1]),
                                        _ptr(fin_score[0]), _ptr(fin_score[1]), _ptr(fin_len[0]), _ptr(fin_len[1]), _ptr(done), _ptr(next_token),
                                        _stream()), "mafed_beam_update")


def seed_word(seed: int, device) -> torch.Tensor:
    """The sampler's seed as one 64-bit word in device memory (int64 storage of the uint64 bit pattern)."""
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must fit a uint64, got {seed}")
    return torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device=device)


def sample_token(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0, *,
                 seed: Optional[torch.Tensor] = None, step: int = 0, uniforms: Optional[torch.Tensor] = None,
                 unfinished: Optional[torch.Tensor] = None, eos_token_id: Optional[int] = None, pad_token_id: int = 0,
                 token: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None, kept: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One drawn token per row of ``logits`` [R, V] (fp32 / bf16, unit column stride): temperature, top-k, top-p and min-p in HF's order,
    then the inverse CDF in ascending token id (mafed_sample_token).  The uniform numbers are ``uniforms`` (fp32 [R]) when given, else
    Philox4x32-10 of (``seed``: the device word of ``seed_word``, row, ``step``).  ``unfinished`` (int64 [R], updated in place): finished
    rows emit ``pad_token_id``, a drawn ``eos_token_id`` clears the flag.  ``logprob`` (fp32 [R]) and ``kept`` (int32 [R]) are optional
    outputs, filled when passed.  Returns ``token`` (int64 [R])."""
    R, V = logits.shape
    assert logits.stride(1) == 1 and (seed is not None or uniforms is not None)
    assert seed is None or (seed.dtype == torch.int64 and seed.numel() == 1)
    assert uniforms is None or (uniforms.dtype == torch.float32 and uniforms.numel() == R and uniforms.is_contiguous())
    assert unfinished is None or (unfinished.dtype == torch.int64 and unfinished.numel() == R and unfinished.is_contiguous())
    assert logprob is None or (logprob.dtype == torch.float32 and logprob.numel() == R and logprob.is_contiguous())
    assert kept is None or (kept.dtype == torch.int32 and kept.numel() == R and kept.is_contiguous())
    if token is None:
        token = torch.empty(R, dtype=torch.int64, device=logits.device)
    assert token.dtype == torch.int64 and token.numel() == R and token.is_contiguous()
    check(_lib.load().mafed_sample_token(_ptr(logits), _dt(logits), logits.stride(0), R, V, float(temperature), int(top_k), float(top_p),
                                         float(min_p), _ptr(seed), int(step), _ptr(uniforms), _ptr(unfinished),
                                         -1 if eos_token_id is None else int(eos_token_id), int(pad_token_id), _ptr(token), _ptr(logprob),
                                         _ptr(kept), _stream()), "mafed_sample_token")
    return token


def gemm_grouped_fuses_sumsq(shapes: Sequence[Tuple[int, int, int]], transA: bool, transB: bool) -> bool:
    """Would ``gemm_grouped`` run these (M, N, K) bf16 -> fp32 products as one persistent launch with the squares of C fused into its
    epilogue?  (host-side query, no launch)"""
    n = len(shapes)
    arr = lambda k: (C.c_int64 * n)(*[int(s[k]) for s in shapes])
    Ms, Ns, Ks = arr(0), arr(1), arr(2)
    return bool(_lib.load().mafed_gemm_grouped_fuses_sumsq(_lib.BF16, int(transA), int(transB), _lib.F32, C.cast(Ms, C.c_void_p),
                                                           C.cast(Ns, C.c_void_p), C.cast(Ks, C.c_void_p), n))


def decode_supported(M: int, h: int, n1: int) -> bool:
    """Shapes served by the fused decode layer kernels (``decode_ln_qkv_fc1`` / ``decode_out``)."""
    return bool(_lib.load().mafed_decode_supported(int(M), int(h), int(n1)))


def decode_ln_qkv_fc1(x: torch.Tensor, ln1_w, ln1_b, ln2_w, ln2_b, eps: float, wqkv: torch.Tensor, bqkv: torch.Tensor,
                      qkv_row: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
    """Decode step, first launch of a layer: ``qkv_row[m] = LN1(x[m]) @ wqkv^T + bqkv`` (a strided [M, 3h] view: the cache row of this
    step) and ``a = gelu(LN2(x[m]) @ w1^T + b1)`` -> a [M, n1] bf16.  x fp32 [M, h]; weights bf16 [N, h]."""
    M, h = x.shape
    n1 = w1.shape[0]
    assert x.dtype == torch.float32 and x.is_contiguous() and wqkv.dtype == torch.bfloat16 and w1.dtype == torch.bfloat16
    assert wqkv.shape == (3 * h, h) and w1.shape[1] == h and wqkv.is_contiguous() and w1.is_contiguous()
    assert qkv_row.shape == (M, 3 * h) and qkv_row.dtype == torch.bfloat16 and qkv_row.stride(1) == 1
    a_out = torch.empty((M, n1), dtype=torch.bfloat16, device=x.device)
    check(_lib.load().mafed_decode_ln_qkv_fc1(_ptr(x), M, h, float(eps), _ptr(ln1_w), _ptr(ln1_b), _ptr(ln2_w), _ptr(ln2_b), _ptr(wqkv),
                                              _ptr(bqkv), _ptr(qkv_row), qkv_row.stride(0), _ptr(w1), _ptr(b1), n1, _ptr(a_out), _stream()),
          "mafed_decode_ln_qkv_fc1")
    return a_out


def decode_ln_linear(x: torch.Tensor, ln_w, ln_b, eps: float, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``LN(x) @ w^T (+ bias)`` for a decode step's M <= 64 rows: final LayerNorm + LM head as one launch.  x fp32 [M, h], w bf16 [N, h]
    -> bf16 [M, N]."""
    M, h = x.shape
    N = w.shape[0]
    assert x.dtype == torch.float32 and x.is_contiguous() and w.dtype == torch.bfloat16 and w.is_contiguous() and w.shape[1] == h
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16 and out.stride(1) == 1
    check(_lib.load().mafed_decode_ln_linear(_ptr(x), M, h, float(eps), _ptr(ln_w), _ptr(ln_b), _ptr(w), _ptr(bias), N, _ptr(out), out.stride(0),
                                             _stream()), "mafed_decode_ln_linear")
    return out


def decode_out_workspace(M: int, h: int, device) -> torch.Tensor:
    """Zero-filled workspace of ``decode_out`` (partial tiles + arrival counters; one per stream).  The counters sit behind the partial
    tiles at an offset that depends on ``ceil(M / 16)``, so a workspace serves calls with the M it was sized for (any M of the same
    ``ceil(M / 16)``), again and again, and the chunked M > 64 form, which is sized as 64 rows and shifts the view for a shorter last block
    itself.  A call with another row-block count would find its counters among the partial tiles: allocate one workspace per M."""
    return torch.zeros(int(_lib.load().mafed_decode_out_workspace_bytes(int(M), int(h))), dtype=torch.uint8, device=device)


def decode_out(x: torch.Tensor, ao: torch.Tensor, act: torch.Tensor, wd: torch.Tensor, bd: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
               workspace: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode step, last launch of a layer: ``x + bd + b2 + ao @ wd^T + act @ w2^T`` -> fp32 [M, h] (``out`` may be ``x``)."""
    M, h = x.shape
    n1 = act.shape[1]
    assert x.dtype == torch.float32 and x.is_contiguous() and ao.shape == (M, h) and ao.is_contiguous() and act.is_contiguous()
    assert ao.dtype == torch.bfloat16 and act.dtype == torch.bfloat16 and wd.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16
    assert wd.shape == (h, h) and w2.shape == (h, n1) and wd.is_contiguous() and w2.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    check(_lib.load().mafed_decode_out(_ptr(x), _ptr(out), M, h, n1, _ptr(ao), _ptr(act), _ptr(wd), _ptr(bd), _ptr(w2), _ptr(b2),
                                       _ptr(workspace), workspace.numel(), _stream()), "mafed_decode_out")
    return out


def embed_concat_fwd(image: torch.Tensor, embed_in: torch.Tensor, input_ids: torch.Tensor, B: int, P: int, T: int) -> torch.Tensor:
    V, h = embed_in.shape
    h0 = torch.empty((B * (P + T), h), dtype=torch.float32, device=embed_in.device)
    check(_lib.load().mafed_embed_concat_fwd(_ptr(image), _dt(image), _ptr(embed_in), _ptr(input_ids), B, P, T, h, V, _ptr(h0),
                                             _stream()), "mafed_embed_concat_fwd")
    return h0


def embed_concat_bwd(dh0, input_ids, B, P, T, h, V, d_embed_in: Optional[torch.Tensor], img_dtype) -> torch.Tensor:
    d_image = torch.empty((B * P, h), dtype=img_dtype, device=dh0.device)
    check(_lib.load().mafed_embed_concat_bwd(_ptr(dh0), _ptr(input_ids), B, P, T, h, V, _ptr(d_image), _dt(d_image),
                                             _ptr(d_embed_in), _stream()), "mafed_embed_concat_bwd")
    return d_image


def _head_args(logits: torch.Tensor, labels: torch.Tensor, poison: Optional[torch.Tensor] = None):
    """What the head-loss wrappers share: ``logits`` [B,T,V] and int64 ``labels`` [B,T], both contiguous, and the optional ``poison`` flag
    (int32 [1], device).  -> (B, T, V, rows), ``rows(*lead)`` a new fp32 [*lead, B, T] buffer on the logits' device."""
    B, T, V = logits.shape
    assert logits.is_contiguous() and labels.is_contiguous() and labels.dtype == torch.int64 and labels.shape == (B, T)
    assert poison is None or (poison.dtype == torch.int32 and poison.numel() == 1)
    return B, T, V, lambda *lead: torch.empty(lead + (B, T), dtype=torch.float32, device=logits.device)


def ce_fwd(logits: torch.Tensor, labels: torch.Tensor, poison: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits [B,T,V] (text positions), labels [B,T] -> (loss[1], lse[B,T]).  ``poison`` (int32 [1], device): a non-zero flag turns the
    loss into NaN (mafed_ce_fwd_guarded: the row-sparse head's overflow flag)."""
    B, T, V, rows = _head_args(logits, labels, poison)
    lse, row_loss = rows(), rows()
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    if poison is None:
        check(_lib.load().mafed_ce_fwd(_ptr(logits), _dt(logits), _ptr(labels), B, T, V, _ptr(lse), _ptr(row_loss), _ptr(loss), _stream()),
              "mafed_ce_fwd")
    else:
        check(_lib.load().mafed_ce_fwd_guarded(_ptr(logits), _dt(logits), _ptr(labels), B, T, V, _ptr(lse), _ptr(row_loss), _ptr(loss),
                                               _ptr(poison), _stream()), "mafed_ce_fwd_guarded")
    return loss, lse


def ce_bwd(logits: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor, gloss: torch.Tensor,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dL/dlogits (pass out=logits for the in-place form)."""
    B, T, V, _ = _head_args(logits, labels)
    if out is None:
        out = torch.empty_like(logits)
    check(_lib.load().mafed_ce_bwd(_ptr(logits), _dt(logits), _ptr(labels), _ptr(lse), B, T, V, _ptr(gloss), _ptr(out), _stream()),
          "mafed_ce_bwd")
    return out


def sqnorm_fwd(logits: torch.Tensor, labels: torch.Tensor, poison: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Squared-norm head objective (mafed_sqnorm_fwd): logits [B,T,V], labels [B,T] -> (J[1], rowsq[B,T]); the rows and the normaliser
    of :func:`ce_fwd`, the label values unused.  ``poison`` as in :func:`ce_fwd`."""
    B, T, V, rows = _head_args(logits, labels, poison)
    rowsq = rows()
    out = torch.empty(1, dtype=torch.float32, device=logits.device)
    check(_lib.load().mafed_sqnorm_fwd(_ptr(logits), _dt(logits), _ptr(labels), B, T, V, _ptr(rowsq), _ptr(out), _ptr(poison), _stream()),
          "mafed_sqnorm_fwd")
    return out, rowsq


def sqnorm_bwd(logits: torch.Tensor, labels: torch.Tensor, dloss: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dJ/dlogits in the logits' dtype, exact zeros on unlabelled rows (``out``: a buffer of its own)."""
    B, T, V, _ = _head_args(logits, labels)
    assert dloss.dtype == torch.float32 and dloss.numel() == 1
    if out is None:
        out = torch.empty_like(logits)
    assert out.dtype == logits.dtype and out.shape == logits.shape and out.is_contiguous()
    check(_lib.load().mafed_sqnorm_bwd(_ptr(logits), _dt(logits), _ptr(labels), B, T, V, _ptr(dloss), _ptr(out), _stream()), "mafed_sqnorm_bwd")
    return out


def _kd_args(student: torch.Tensor, teacher: torch.Tensor, labels: torch.Tensor, poison: Optional[torch.Tensor] = None):
    """:func:`_head_args` of the student's logits, with a teacher of the same shape and dtype"""
    if teacher.shape != student.shape or teacher.dtype != student.dtype:
        raise ValueError(f"teacher logits {tuple(teacher.shape)} {teacher.dtype} do not match the student's {tuple(student.shape)} {student.dtype}")
    assert teacher.is_contiguous()
    return _head_args(student, labels, poison)


def ce_kd_fwd(student: torch.Tensor, teacher: torch.Tensor, labels: torch.Tensor, tau: float, lam: float,
              poison: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """LwF head loss (mafed_ce_kd_fwd): student / teacher logits [B,T,V] of the same rows, labels [B,T] ->
    (out3 = [CE + lam tau^2 KD, CE, KD], lse3 [3,B,T] = lse(s), lse(s / tau), lse(t / tau)).  ``poison`` as in :func:`ce_fwd`."""
    B, T, V, rows = _kd_args(student, teacher, labels, poison)
    lse3, row = rows(3), rows(2)
    out3 = torch.empty(3, dtype=torch.float32, device=student.device)
    check(_lib.load().mafed_ce_kd_fwd(_ptr(student), _ptr(teacher), _dt(student), _ptr(labels), B, T, V, float(tau), float(lam), _ptr(lse3),
                                      _ptr(row[0]), _ptr(row[1]), _ptr(out3), _ptr(poison), _stream()), "mafed_ce_kd_fwd")
    return out3, lse3


def ce_kd_bwd(student: torch.Tensor, teacher: torch.Tensor, labels: torch.Tensor, lse3: torch.Tensor, tau: float, lam: float,
              gloss: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dL/d(student logits) of :func:`ce_kd_fwd`: the cross-entropy and the distillation gradient, one pass (``out``: a buffer of its own)."""
    B, T, V, _ = _kd_args(student, teacher, labels)
    assert lse3.shape == (3, B, T) and lse3.dtype == torch.float32 and lse3.is_contiguous()
    if out is None:
        out = torch.empty_like(student)
    assert out.data_ptr() != student.data_ptr() and out.data_ptr() != teacher.data_ptr()
    check(_lib.load().mafed_ce_kd_bwd(_ptr(student), _ptr(teacher), _dt(student), _ptr(labels), _ptr(lse3), B, T, V, float(tau), float(lam),
                                      _ptr(gloss), _ptr(out), _stream()), "mafed_ce_kd_bwd")
    return out


def _anchor_args(student: torch.Tensor, store: torch.Tensor, mem_index: torch.Tensor, labels: torch.Tensor, poison: Optional[torch.Tensor] = None):
    """:func:`_head_args` of the student's logits, with a store [n_mem, A, V] of the same dtype and V and an int64 ``mem_index`` [B]
    -> (B, T, V, rows, n_mem, A)"""
    B, T, V, rows = _head_args(student, labels, poison)
    if store.dim() != 3 or store.shape[2] != V or store.dtype != student.dtype or store.device != student.device or not store.is_contiguous():
        raise ValueError(f"store {tuple(store.shape)} {store.dtype} does not match head logits {tuple(student.shape)} {student.dtype} "
                         "(a contiguous [n_mem, A, V] tensor of the same dtype, V and device)")
    if mem_index.dtype != torch.int64 or mem_index.shape != (B,) or mem_index.device != student.device or not mem_index.is_contiguous():
        raise ValueError(f"mem_index must be a contiguous int64 [{B}] tensor on the logits' device, got {tuple(mem_index.shape)} {mem_index.dtype}")
    return B, T, V, rows, store.shape[0], store.shape[1]


def ce_mse_fwd(logits: torch.Tensor, store: torch.Tensor, mem_index: torch.Tensor, labels: torch.Tensor, alpha: float, beta: float,
               poison: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """DER++ head loss (mafed_ce_mse_fwd): student logits [B,T,V], ``store`` [n_mem, A, V] of stored answer logits, ``mem_index`` int64 [B]
    (the stored sample of each batch row), labels [B,T] -> (out3 = [beta CE + alpha MSE, CE, MSE], lse [B,T]).  Labelled row (b, t) is
    held against ``store[mem_index[b], rank of t among b's labelled rows]``, read in place.  ``poison`` as in :func:`ce_fwd`."""
    B, T, V, rows, n_mem, A = _anchor_args(logits, store, mem_index, labels, poison)
    lse, row = rows(), rows(2)
    out3 = torch.empty(3, dtype=torch.float32, device=logits.device)
    check(_lib.load().mafed_ce_mse_fwd(_ptr(logits), _ptr(store), _dt(logits), _ptr(labels), _ptr(mem_index), B, T, V, n_mem, A, float(alpha),
                                       float(beta), _ptr(lse), _ptr(row[0]), _ptr(row[1]), _ptr(out3), _ptr(poison), _stream()), "mafed_ce_mse_fwd")
    return out3, lse


def ce_mse_bwd(logits: torch.Tensor, store: torch.Tensor, mem_index: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor, alpha: float,
               beta: float, gloss: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dL/d(student logits) of :func:`ce_mse_fwd`: the cross-entropy and the squared-distance gradient, one pass (``out``: a buffer of its own)."""
    B, T, V, _, n_mem, A = _anchor_args(logits, store, mem_index, labels)
    assert lse.shape == (B, T) and lse.dtype == torch.float32 and lse.is_contiguous()
    if out is None:
        out = torch.empty_like(logits)
    assert out.shape == logits.shape and out.dtype == logits.dtype and out.is_contiguous() and out.data_ptr() != logits.data_ptr()
    check(_lib.load().mafed_ce_mse_bwd(_ptr(logits), _ptr(store), _dt(logits), _ptr(labels), _ptr(mem_index), _ptr(lse), B, T, V, n_mem, A,
                                       float(alpha), float(beta), _ptr(gloss), _ptr(out), _stream()), "mafed_ce_mse_bwd")
    return out


def distill_fwd(s: torch.Tensor, t, attention_mask: torch.Tensor, P: int, cosine: bool = False,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> out[4] = {lang_sum, vision_sum, n_lang, n_vision}; ``t`` a dense fp32 [B, S, h] tensor or ``TeacherRows``"""
    B, S, h = s.shape
    assert s.dtype == torch.float32 and s.is_contiguous()
    tp, tdt, tix = _teacher(t, B, S, h)
    lib = _lib.load()
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=s.device)
    nb = lib.mafed_distill_workspace_bytes(B * S)
    ws = workspace(s.device).get(nb)
    check(lib.mafed_distill_fwd_indexed(_ptr(s), tp, tdt, tix, _ptr(attention_mask), B, S, P, h, int(cosine), _ptr(out), _ptr(ws), ws.numel(),
                                        _stream()), "mafed_distill_fwd")
    return out


def distill_bwd(s, t, attention_mask, P: int, coef: torch.Tensor, cosine: bool = False, out: Optional[torch.Tensor] = None,
                accumulate: bool = False) -> torch.Tensor:
    B, S, h = s.shape
    if out is None:
        out = torch.empty_like(s)
        accumulate = False
    tp, tdt, tix = _teacher(t, B, S, h)
    check(_lib.load().mafed_distill_bwd_indexed(_ptr(s), tp, tdt, tix, _ptr(attention_mask), B, S, P, h, int(cosine), _ptr(coef), _ptr(out),
                                                int(accumulate), _stream()), "mafed_distill_bwd")
    return out


def distill_combine(sums: torch.Tensor, layer_coeff: torch.Tensor, mode: int, lang_weight: float = 0.5,
                    lang_weight_vec: Optional[torch.Tensor] = None):
    """sums [nl,4] -> (loss [1], per_layer [nl], modality [nl,2], inject [nl,4]) in one launch (mafed_distill_combine)."""
    nl = sums.shape[0]
    assert sums.dtype == torch.float32 and sums.is_contiguous() and layer_coeff.dtype == torch.float32 and layer_coeff.numel() == nl
    dev = sums.device
    out = torch.empty(1 + nl + 2 * nl + 4 + 4 * nl, dtype=torch.float32, device=dev)  # one allocation; inject 16-byte aligned
    loss, per_layer, modality = out[0:1], out[1:1 + nl], out[1 + nl:1 + 3 * nl].view(nl, 2)
    o = (1 + 3 * nl + 3) // 4 * 4
    inject = out[o:o + 4 * nl].view(nl, 4)
    check(_lib.load().mafed_distill_combine(_ptr(sums), nl, _ptr(layer_coeff), int(mode), float(lang_weight), _ptr(lang_weight_vec), _ptr(loss),
                                            _ptr(per_layer), _ptr(modality), _ptr(inject), _stream()), "mafed_distill_combine")
    return loss, per_layer, modality, inject


def distill_cls_fwd(s, t) -> torch.Tensor:
    B, S, h = s.shape
    out = torch.empty(1, dtype=torch.float32, device=s.device)
    tp, tdt, tix = _teacher(t, B, S, h)
    check(_lib.load().mafed_distill_cls_fwd_indexed(_ptr(s), tp, tdt, tix, B, S, h, _ptr(out), _stream()), "mafed_distill_cls_fwd")
    return out


def distill_cls_bwd(s, t, coef) -> torch.Tensor:
    B, S, h = s.shape
    out = torch.empty_like(s)
    tp, tdt, tix = _teacher(t, B, S, h)
    check(_lib.load().mafed_distill_cls_bwd_indexed(_ptr(s), tp, tdt, tix, B, S, h, _ptr(coef), _ptr(out), 0, _stream()), "mafed_distill_cls_bwd")
    return out


def _flat_f32(*ts: torch.Tensor) -> None:
    """The flat-buffer passes take contiguous one-dimensional fp32 tensors of one length."""
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 1 and t.numel() == ts[0].numel() for t in ts)


def ewc_penalty_fwd(p: torch.Tensor, p_old: torch.Tensor, fisher: torch.Tensor, half_lambda: float,
                    out: Optional[torch.Tensor] = None, beta: float = 0.0) -> torch.Tensor:
    """out[0] = beta * out[0] + half_lambda * sum fisher * (p - p_old)^2 over flat fp32 buffers."""
    _flat_f32(p, p_old, fisher)
    lib = _lib.load()
    if out is None:
        out = torch.zeros(1, dtype=torch.float32, device=p.device)
    ws = workspace(p.device).get(lib.mafed_ewc_workspace_bytes(p.numel()))
    check(lib.mafed_ewc_penalty_fwd(_ptr(p), _ptr(p_old), _ptr(fisher), p.numel(), float(half_lambda), float(beta), _ptr(out), _ptr(ws),
                                    ws.numel(), _stream()), "mafed_ewc_penalty_fwd")
    return out


def ewc_penalty_bwd_(p: torch.Tensor, p_old: torch.Tensor, fisher: torch.Tensor, lam: float, coef: torch.Tensor, grad: torch.Tensor) -> None:
    """grad += coef[0] * lam * fisher * (p - p_old)"""
    _flat_f32(p, p_old, fisher, grad)
    assert coef.dtype == torch.float32
    check(_lib.load().mafed_ewc_penalty_bwd(_ptr(p), _ptr(p_old), _ptr(fisher), p.numel(), float(lam), _ptr(coef), _ptr(grad), _stream()),
          "mafed_ewc_penalty_bwd")


def agem_blocks(n: int) -> int:
    """Number of sum-of-squares partials ``agem_project`` writes for n elements."""
    return int(_lib.load().mafed_agem_blocks(int(n)))


def agem_dots(g: torch.Tensor, r: torch.Tensor, stats4: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> stats4 = {sum g r, sum r r, alpha, violated} over flat fp32 buffers (A-GEM: alpha = dot / rsq if dot < 0 and rsq > 0, else 0)."""
    _flat_f32(g, r)
    lib = _lib.load()
    if stats4 is None:
        stats4 = torch.empty(4, dtype=torch.float32, device=g.device)
    assert stats4.dtype == torch.float32 and stats4.numel() == 4 and stats4.is_contiguous()
    ws = workspace(g.device).get(lib.mafed_agem_workspace_bytes(g.numel()))
    check(lib.mafed_agem_dots(_ptr(g), _ptr(r), g.numel(), _ptr(stats4), _ptr(ws), ws.numel(), _stream()), "mafed_agem_dots")
    return stats4


def agem_project(g: torch.Tensor, r: torch.Tensor, stats4: torch.Tensor, out: Optional[torch.Tensor] = None,
                 sumsq_partials: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = g - stats4[2] * r (alpha is read on the device; 0 copies g bit for bit); ``out`` may be ``r``.  ``sumsq_partials``
    [>= agem_blocks(n)] receives the sum-of-squares partials of ``out`` for ``gradnorm_finish``."""
    _flat_f32(g, r)
    if out is None:
        out = torch.empty_like(g)
    _flat_f32(g, out)
    assert stats4.dtype == torch.float32 and stats4.numel() == 4 and stats4.is_contiguous()
    if sumsq_partials is not None:
        assert sumsq_partials.dtype == torch.float32 and sumsq_partials.is_contiguous() and sumsq_partials.numel() >= agem_blocks(g.numel())
    check(_lib.load().mafed_agem_project(_ptr(g), _ptr(r), _ptr(out), g.numel(), _ptr(stats4), _ptr(sumsq_partials), _stream()),
          "mafed_agem_project")
    return out


GEM_MAX_REFS = 8


def gem_blocks(n: int) -> int:
    """Number of sum-of-squares partials ``gem_project`` writes for n elements."""
    return int(_lib.load().mafed_gem_blocks(int(n)))


def _gem_refs(g: torch.Tensor, refs: Sequence[torch.Tensor]):
    """The host array of K device pointers the GEM passes take.  K outside 1 .. 8 is left to the library to refuse."""
    refs = list(refs)
    _flat_f32(g, *refs)
    return (C.c_void_p * max(len(refs), 1))(*[_ptr(r) for r in refs]), len(refs)


def gem_gram(g: torch.Tensor, refs: Sequence[torch.Tensor], gram64: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> gram64 [(K + 1), (K + 1)] fp64 on the device: the inner products of x_0 = g and x_k = refs[k - 1] over flat fp32 buffers."""
    arr, K = _gem_refs(g, refs)
    lib = _lib.load()
    if gram64 is None:
        gram64 = torch.empty((K + 1, K + 1), dtype=torch.float64, device=g.device)
    assert gram64.dtype == torch.float64 and gram64.numel() == (K + 1) * (K + 1) and gram64.is_contiguous()
    ws = workspace(g.device).get(lib.mafed_gem_workspace_bytes(g.numel(), K))
    check(lib.mafed_gem_gram(_ptr(g), arr, K, g.numel(), _ptr(gram64), _ptr(ws), ws.numel(), _stream()), "mafed_gem_gram")
    return gram64


def gem_solve(gram64: torch.Tensor, K: int, margin: float, eps: float, stats12: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> stats12 = {v_0 .. v_7, violated, support size, 0, 0}: GEM's dual quadratic programme on the Gram of ``gem_gram``, solved
    exactly on the device (v_k >= margin, eps on the diagonal of P)."""
    K = int(K)
    assert gram64.dtype == torch.float64 and gram64.is_contiguous() and (not 1 <= K <= GEM_MAX_REFS or gram64.numel() == (K + 1) * (K + 1))
    if stats12 is None:
        stats12 = torch.empty(12, dtype=torch.float32, device=gram64.device)
    assert stats12.dtype == torch.float32 and stats12.numel() == 12 and stats12.is_contiguous()
    check(_lib.load().mafed_gem_solve(_ptr(gram64), K, float(margin), float(eps), _ptr(stats12), _stream()), "mafed_gem_solve")
    return stats12


def gem_project(g: torch.Tensor, refs: Sequence[torch.Tensor], stats12: torch.Tensor, out: Optional[torch.Tensor] = None,
                sumsq_partials: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = g + sum_k stats12[k] * refs[k] where stats12[8] says violated (read on the device), else g bit for bit; ``out`` may be
    ``g`` or any of ``refs``.  ``sumsq_partials`` [>= gem_blocks(n)] receives the sum-of-squares partials of ``out`` for
    ``gradnorm_finish``."""
    arr, K = _gem_refs(g, refs)
    if out is None:
        out = torch.empty_like(g)
    _flat_f32(g, out)
    assert stats12.dtype == torch.float32 and stats12.numel() == 12 and stats12.is_contiguous()
    if sumsq_partials is not None:
        assert sumsq_partials.dtype == torch.float32 and sumsq_partials.is_contiguous() and sumsq_partials.numel() >= gem_blocks(g.numel())
    check(_lib.load().mafed_gem_project(_ptr(g), arr, K, _ptr(out), g.numel(), _ptr(stats12), _ptr(sumsq_partials), _stream()),
          "mafed_gem_project")
    return out


def si_blocks(n: int) -> int:
    """Number of partials of each kind ``si_stash`` writes for n elements."""
    return int(_lib.load().mafed_si_blocks(int(n)))


def si_stash(g: torch.Tensor, p: torch.Tensor, omega: Optional[torch.Tensor], anchor: Optional[torch.Tensor], two_c: float,
             stash_g: torch.Tensor, stash_p: torch.Tensor, sumsq_partials: torch.Tensor, pen_partials: torch.Tensor) -> None:
    """stash_g = g, stash_p = p (bit copies); with ``omega`` / ``anchor``: g += two_c * omega * (p - anchor) in place.  ``sumsq_partials``
    [>= si_blocks(n)] receives the sum-of-squares partials of the g it leaves (``gradnorm_finish``), ``pen_partials`` those of
    sum omega (p - anchor)^2 (``si_penalty_finish``)."""
    _flat_f32(g, p, stash_g, stash_p, *([] if omega is None else [omega, anchor]))
    assert (omega is None) == (anchor is None)
    nb = si_blocks(g.numel())
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= nb for t in (sumsq_partials, pen_partials))
    check(_lib.load().mafed_si_stash(_ptr(g), _ptr(p), _ptr(omega), _ptr(anchor), g.numel(), float(two_c), _ptr(stash_g), _ptr(stash_p),
                                     _ptr(sumsq_partials), _ptr(pen_partials), _stream()), "mafed_si_stash")


def si_penalty_finish(pen_partials: torch.Tensor, c: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[0] = c * sum of the penalty partials (folded in double, fixed order)."""
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=pen_partials.device)
    assert pen_partials.dtype == torch.float32 and pen_partials.is_contiguous() and out.dtype == torch.float32 and out.numel() == 1
    check(_lib.load().mafed_si_penalty_finish(_ptr(pen_partials), pen_partials.numel(), float(c), _ptr(out), _stream()), "mafed_si_penalty_finish")
    return out


def si_accumulate_(stash_g: torch.Tensor, stash_p: torch.Tensor, p: torch.Tensor, w: torch.Tensor) -> None:
    """w -= stash_g * (p - stash_p) where p != stash_p; an unmoved element keeps its w bit for bit."""
    _flat_f32(stash_g, stash_p, p, w)
    check(_lib.load().mafed_si_accumulate(_ptr(stash_g), _ptr(stash_p), _ptr(p), _ptr(w), w.numel(), _stream()), "mafed_si_accumulate")


def si_consolidate_(p: torch.Tensor, anchor: torch.Tensor, w: torch.Tensor, omega: torch.Tensor, xi: float) -> None:
    """omega = max(omega + w / ((p - anchor)^2 + xi), 0); anchor = p; w = 0."""
    _flat_f32(p, anchor, w, omega)
    check(_lib.load().mafed_si_consolidate(_ptr(p), _ptr(anchor), _ptr(w), _ptr(omega), p.numel(), float(xi), _stream()), "mafed_si_consolidate")


def mas_blocks(n: int) -> int:
    """Number of partials of each kind ``mas_penalty_`` writes for n elements (== ``si_blocks(n)``)."""
    return int(_lib.load().mafed_mas_blocks(int(n)))


def mas_accumulate_(g: torch.Tensor, acc: torch.Tensor, weight: float) -> None:
    """acc = fma(weight, |g|, acc)."""
    _flat_f32(g, acc)
    check(_lib.load().mafed_mas_accumulate(_ptr(g), _ptr(acc), g.numel(), float(weight), _stream()), "mafed_mas_accumulate")


def mas_consolidate_(acc: torch.Tensor, omega: torch.Tensor, p: torch.Tensor, anchor: torch.Tensor, inv_seen: float, alpha: float,
                     first: bool) -> None:
    """omega = inv_seen * acc (``first``; omega is not read) or alpha * omega + (1 - alpha) * inv_seen * acc; anchor = p; acc = 0."""
    _flat_f32(acc, omega, p, anchor)
    check(_lib.load().mafed_mas_consolidate(_ptr(acc), _ptr(omega), _ptr(p), _ptr(anchor), p.numel(), float(inv_seen), float(alpha),
                                            int(bool(first)), _stream()), "mafed_mas_consolidate")


def mas_penalty_(g: torch.Tensor, p: torch.Tensor, omega: torch.Tensor, anchor: torch.Tensor, two_c: float, sumsq_partials: torch.Tensor,
                 pen_partials: torch.Tensor) -> None:
    """g += two_c * omega * (p - anchor) in place.  ``sumsq_partials`` [>= mas_blocks(n)] receives the sum-of-squares partials of the g it
    leaves (``gradnorm_finish``), ``pen_partials`` those of sum omega (p - anchor)^2 (``si_penalty_finish``)."""
    _flat_f32(g, p, omega, anchor)
    nb = mas_blocks(g.numel())
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= nb for t in (sumsq_partials, pen_partials))
    check(_lib.load().mafed_mas_penalty(_ptr(g), _ptr(p), _ptr(omega), _ptr(anchor), g.numel(), float(two_c), _ptr(sumsq_partials),
                                        _ptr(pen_partials), _stream()), "mafed_mas_penalty")


PACKNET_BINS = 2048   # uint32 bins per segment of the prune's histogram workspace


def packnet_blocks(n: int) -> int:
    """Number of sum-of-squares partials ``packnet_mask_grad_`` writes for n elements."""
    return int(_lib.load().mafed_packnet_blocks(int(n)))


def _packnet_flat(x: torch.Tensor, owner: torch.Tensor, shadow: Optional[torch.Tensor] = None, anchor: Optional[torch.Tensor] = None) -> None:
    """fp32 buffers, the uint8 owner map and the bf16 shadow: contiguous, one-dimensional, of one length."""
    _flat_f32(x, *([] if anchor is None else [anchor]))
    assert owner.dtype == torch.uint8 and owner.is_contiguous() and owner.dim() == 1 and owner.numel() == x.numel()
    assert shadow is None or (shadow.dtype == torch.bfloat16 and shadow.is_contiguous() and shadow.dim() == 1 and shadow.numel() == x.numel())


def packnet_mask_grad_(g: torch.Tensor, owner: torch.Tensor, task: int, sumsq_partials: torch.Tensor) -> None:
    """g = owner == task ? g : +0.0 in place.  ``sumsq_partials`` [>= packnet_blocks(n)] receives the sum-of-squares partials of the g it
    leaves (``gradnorm_finish``)."""
    _packnet_flat(g, owner)
    assert sumsq_partials.dtype == torch.float32 and sumsq_partials.is_contiguous() and sumsq_partials.numel() >= packnet_blocks(g.numel())
    check(_lib.load().mafed_packnet_mask_grad(_ptr(g), _ptr(owner), g.numel(), int(task), _ptr(sumsq_partials), _stream()), "mafed_packnet_mask_grad")


def packnet_hold_(p: torch.Tensor, shadow: Optional[torch.Tensor], owner: torch.Tensor, anchor: torch.Tensor, task: int) -> None:
    """Where owner != task: p = anchor, shadow = bf16(anchor).  Nothing else is written."""
    _packnet_flat(p, owner, shadow, anchor)
    check(_lib.load().mafed_packnet_hold(_ptr(p), _ptr(shadow), _ptr(owner), _ptr(anchor), p.numel(), int(task), _stream()), "mafed_packnet_hold")


def packnet_view_(p: torch.Tensor, shadow: Optional[torch.Tensor], owner: torch.Tensor, k: int) -> None:
    """Where owner > k: p = +0.0, shadow = 0.  Nothing else is written."""
    _packnet_flat(p, owner, shadow)
    check(_lib.load().mafed_packnet_view(_ptr(p), _ptr(shadow), _ptr(owner), p.numel(), int(k), _stream()), "mafed_packnet_view")


def packnet_select_blocks(max_length: int, n_segments: int) -> int:
    """Blocks per segment of the prune's launches: one per 1024 fp32 vectors of the longest segment, and about 4096 blocks in all at most
    (every block adds its non-empty bins to the segment's histogram)."""
    want = (int(max_length) // 4 + 1 + 1023) // 1024
    return max(1, min(want, 4096 // max(1, int(n_segments))))


def _packnet_tables(segments: torch.Tensor, state: torch.Tensor, stats: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None) -> int:
    assert segments.dtype == torch.int64 and segments.is_contiguous() and segments.dim() == 2 and segments.size(1) == 2
    n_seg = segments.size(0)
    for t in (state, stats):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.numel() >= 4 * n_seg)
    assert hist is None or (hist.dtype == torch.int32 and hist.is_contiguous() and hist.numel() >= PACKNET_BINS * n_seg)
    return n_seg


def packnet_hist(p: torch.Tensor, owner: torch.Tensor, segments: torch.Tensor, blocks_per_segment: int, task: int, radix_pass: int,
                 state: torch.Tensor, hist: torch.Tensor) -> None:
    """hist[s][bin] = number of elements of segment s with owner == task whose bits above digit ``radix_pass`` equal the prefix in state."""
    _packnet_flat(p, owner)
    n_seg = _packnet_tables(segments, state, hist=hist)
    check(_lib.load().mafed_packnet_hist(_ptr(p), _ptr(owner), p.numel(), _ptr(segments), n_seg, int(blocks_per_segment), int(task), int(radix_pass),
                                         _ptr(state), _ptr(hist), _stream()), "mafed_packnet_hist")


def packnet_scan(hist: torch.Tensor, n_segments: int, radix_pass: int, fraction: float, state: torch.Tensor, stats: torch.Tensor) -> None:
    """Per segment: the bin that holds the wanted rank -> the extended prefix and the remaining rank in state; pass 0 derives m and k."""
    assert hist.dtype == torch.int32 and hist.numel() >= PACKNET_BINS * n_segments and state.numel() >= 4 * n_segments and stats.numel() >= 4 * n_segments
    assert state.dtype == torch.int64 and stats.dtype == torch.int64
    check(_lib.load().mafed_packnet_scan(_ptr(hist), int(n_segments), int(radix_pass), float(fraction), _ptr(state), _ptr(stats), _stream()),
          "mafed_packnet_scan")


def packnet_apply_(p: torch.Tensor, shadow: Optional[torch.Tensor], owner: torch.Tensor, anchor: torch.Tensor, segments: torch.Tensor,
                   blocks_per_segment: int, task: int, state: torch.Tensor, stats: torch.Tensor) -> None:
    """Where owner == task and |p| <= tau of the segment: p = anchor = +0.0, shadow = 0, owner = task + 1; stats[s][2] = their number."""
    _packnet_flat(p, owner, shadow, anchor)
    n_seg = _packnet_tables(segments, state, stats)
    check(_lib.load().mafed_packnet_apply(_ptr(p), _ptr(shadow), _ptr(owner), _ptr(anchor), p.numel(), _ptr(segments), n_seg, int(blocks_per_segment),
                                          int(task), _ptr(state), _ptr(stats), _stream()), "mafed_packnet_apply")


def packnet_prune_(p: torch.Tensor, shadow: Optional[torch.Tensor], owner: torch.Tensor, anchor: torch.Tensor, segments: torch.Tensor,
                   blocks_per_segment: int, task: int, fraction: float, state: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None,
                   stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The whole prune of every segment (int64 [S, 2] = {offset, length} on the device): three histogram + scan passes, then the apply pass;
    seven launches, nothing read back.  -> stats, int64 [S, 4] = {m, k, pruned, pattern of tau} on the device."""
    n_seg, dev = segments.size(0), p.device
    state = torch.zeros(n_seg, 4, dtype=torch.int64, device=dev) if state is None else state
    stats = torch.zeros(n_seg, 4, dtype=torch.int64, device=dev) if stats is None else stats
    hist = torch.zeros(n_seg, PACKNET_BINS, dtype=torch.int32, device=dev) if hist is None else hist
    for radix_pass in range(3):
        packnet_hist(p, owner, segments, blocks_per_segment, task, radix_pass, state, hist)
        packnet_scan(hist, n_seg, radix_pass, fraction, state, stats)
    packnet_apply_(p, shadow, owner, anchor, segments, blocks_per_segment, task, state, stats)
    return stats


MERGE_RULES = {"sum": 0, "magmax": 1, "ties": 2}   # MAFED_MERGE_* of include/mafed_hip.h


def _merge_flat(*ts: Optional[torch.Tensor], shadow: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None) -> int:
    """fp32 buffers of one length n, the bf16 shadow [n] and the byte counters [n, 2]: contiguous.  A mismatch is refused with
    ``MafedHipError`` in front of any launch, like a misaligned pointer."""
    ts = [t for t in ts if t is not None]
    n = ts[0].numel()
    ok = all(t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 1 and t.numel() == n for t in ts)
    ok = ok and (shadow is None or (shadow.dtype == torch.bfloat16 and shadow.is_contiguous() and shadow.dim() == 1 and shadow.numel() == n))
    ok = ok and (counts is None or (counts.dtype == torch.uint8 and counts.is_contiguous() and counts.shape == (n, 2)))
    if not ok:
        raise _lib.MafedHipError("merge: the flat buffers must be contiguous, one-dimensional and of one length (fp32; bf16 shadow [n]; "
                                 "uint8 counts [n, 2])")
    return n


def merge_select_blocks(max_length: int) -> int:
    """Blocks per segment of the TIES launches: one per 1024 fp32 vectors of the longest segment, 512 at most.  Unlike PackNet's layer
    matrices the tensors of a model differ in length by orders of magnitude; a block with no vector of its segment leaves at once."""
    return max(1, min((int(max_length) // 4 + 1 + 1023) // 1024, 512))


def merge_fold_(theta: torch.Tensor, base: torch.Tensor, acc: torch.Tensor, rule: str) -> None:
    """tau = theta - base; ``"sum"``: acc += tau; ``"magmax"``: acc = |tau| > |acc| ? tau : acc.  Each operation rounded once."""
    if rule not in ("sum", "magmax"):
        raise ValueError("merge_fold_: rule must be 'sum' or 'magmax', not %r" % (rule,))
    n = _merge_flat(theta, base, acc)
    check(_lib.load().mafed_merge_fold(_ptr(theta), _ptr(base), _ptr(acc), n, MERGE_RULES[rule], _stream()), "mafed_merge_fold")


def merge_ties_hist(theta: torch.Tensor, base: torch.Tensor, segments: torch.Tensor, blocks_per_segment: int, radix_pass: int,
                    state: torch.Tensor, hist: torch.Tensor) -> None:
    """hist[s][bin] = number of elements of segment s whose pattern of |theta - base| has the prefix in state above digit ``radix_pass``."""
    n = _merge_flat(theta, base)
    n_seg = _packnet_tables(segments, state, hist=hist)
    check(_lib.load().mafed_merge_ties_hist(_ptr(theta), _ptr(base), n, _ptr(segments), n_seg, int(blocks_per_segment), int(radix_pass), _ptr(state),
                                            _ptr(hist), _stream()), "mafed_merge_ties_hist")


def merge_ties_fold_pass_(theta: torch.Tensor, base: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, counts: torch.Tensor,
                           segments: torch.Tensor, blocks_per_segment: int, state: torch.Tensor, stats: torch.Tensor) -> None:
    """The fold pass alone, with the threshold the third scan left in ``state``: on kept elements pos / neg += tau and their counter += 1;
    stats[s][2] = the number kept."""
    n = _merge_flat(theta, base, pos, neg, counts=counts)
    n_seg = _packnet_tables(segments, state, stats)
    check(_lib.load().mafed_merge_ties_fold(_ptr(theta), _ptr(base), _ptr(pos), _ptr(neg), _ptr(counts), n, _ptr(segments), n_seg,
                                            int(blocks_per_segment), _ptr(state), _ptr(stats), _stream()), "mafed_merge_ties_fold")


def merge_ties_fold_(theta: torch.Tensor, base: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, counts: torch.Tensor, segments: torch.Tensor,
                     blocks_per_segment: int, drop: float, state: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None,
                     stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One TIES fold of every segment (int64 [S, 2] = {offset, length} on the device): three histogram + scan passes find the
    floor(drop * m)-th smallest |theta - base| of each, then the fold pass; seven launches, nothing read back.
    -> stats, int64 [S, 4] = {m, r, kept, pattern of the threshold} on the device."""
    _merge_flat(theta, base, pos, neg, counts=counts)   # (in front of the first launch)
    n_seg, dev = segments.size(0), theta.device
    state = torch.zeros(n_seg, 4, dtype=torch.int64, device=dev) if state is None else state
    stats = torch.zeros(n_seg, 4, dtype=torch.int64, device=dev) if stats is None else stats
    hist = torch.zeros(n_seg, PACKNET_BINS, dtype=torch.int32, device=dev) if hist is None else hist
    for radix_pass in range(3):
        merge_ties_hist(theta, base, segments, blocks_per_segment, radix_pass, state, hist)
        packnet_scan(hist, n_seg, radix_pass, drop, state, stats)
    merge_ties_fold_pass_(theta, base, pos, neg, counts, segments, blocks_per_segment, state, stats)
    return stats


def merge_apply_(p: torch.Tensor, shadow: Optional[torch.Tensor], base: torch.Tensor, acc: torch.Tensor, rule: str, scaling: float,
                 neg: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None) -> None:
    """p = base + scaling * d (product and sum rounded separately), shadow = bf16(p).  d = acc for ``"sum"`` and ``"magmax"``; for
    ``"ties"`` (acc = pos, with ``neg`` and ``counts``) the mean of the elected sign: pos / npos where pos + neg > 0, neg / nneg where
    it is < 0, +0.0 otherwise."""
    if rule not in MERGE_RULES:
        raise ValueError("merge_apply_: unknown rule %r" % (rule,))
    if (rule == "ties") != (neg is not None and counts is not None) or (neg is None) != (counts is None):
        raise _lib.MafedHipError("merge_apply_: neg and counts come with the ties rule, and only with it")
    n = _merge_flat(p, base, acc, neg, shadow=shadow, counts=counts)
    check(_lib.load().mafed_merge_apply(_ptr(p), _ptr(shadow), _ptr(base), _ptr(acc), _ptr(neg), _ptr(counts), n, MERGE_RULES[rule], float(scaling),
                                        _stream()), "mafed_merge_apply")


def cka_pool(hidden: Sequence[torch.Tensor], attention_mask: torch.Tensor, P: int, out: torch.Tensor, rows: Optional[torch.Tensor] = None) -> None:
    """out[0, l, rows[b]] = mean of hidden[l][b, :P]; out[1, l, rows[b]] = mean of the last sum(attention_mask[b]) rows of hidden[l][b]
    (fp32 hidden states [B, S, h], text mask [B, T], out fp32 [2, L, n, h])."""
    L = len(hidden)
    B, S, h = hidden[0].shape
    T = attention_mask.shape[1]
    assert all(x.shape == (B, S, h) and x.dtype == torch.float32 and x.is_contiguous() for x in hidden)
    assert attention_mask.dtype == torch.int64 and attention_mask.shape == (B, T) and attention_mask.is_contiguous()
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and out.shape[0] == 2 and out.shape[1] == L and out.shape[3] == h
    if rows is not None:
        assert rows.dtype == torch.int64 and rows.shape == (B,) and rows.is_contiguous()
    ptrs = (C.c_void_p * L)(*[_ptr(x) for x in hidden])
    check(_lib.load().mafed_cka_pool(ptrs, L, B, S, int(P), h, _ptr(attention_mask), T, _ptr(rows), out.shape[2], _ptr(out), _stream()),
          "mafed_cka_pool")


def cka_stats(X: torch.Tensor, row_norms: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """fp64 column means [G, h] and centred squared row norms [G, n] of G fp32 feature sets X [G, n, h] (or one set [n, h])."""
    assert X.dtype == torch.float32 and X.dim() in (2, 3) and X.stride(-1) == 1
    X3 = X if X.dim() == 3 else X.unsqueeze(0)
    G, n, h = X3.shape
    lib = _lib.load()
    mean = torch.empty((G, h), dtype=torch.float64, device=X.device)
    rsq = torch.empty((G, n), dtype=torch.float64, device=X.device) if row_norms else None
    ws = workspace(X.device).get(lib.mafed_cka_stats_workspace_bytes(G, n, h))
    check(lib.mafed_cka_stats(_ptr(X3), G, n, h, X3.stride(1), X3.stride(0), _ptr(mean), _ptr(rsq), _ptr(ws), ws.numel(), _stream()),
          "mafed_cka_stats")
    return mean, rsq


def cka_hsic(products: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[p] = ||(X - 1 mean_x^T)^T (Y - 1 mean_y^T)||_F^2 for every (X [n, hx], mean_x [hx], Y [n, hy], mean_y [hy]) in ``products``,
    fp64 [len(products)]; passing the same tensors as X and Y makes a self term (upper-triangle tiles only)."""
    descs = (_lib.CkaProduct * max(1, len(products)))()
    dev = None
    for i, (X, mx, Y, my) in enumerate(products):
        assert X.dtype == torch.float32 and Y.dtype == torch.float32 and X.dim() == 2 and Y.dim() == 2 and X.shape[0] == Y.shape[0]
        assert X.stride(1) == 1 and Y.stride(1) == 1
        assert mx.dtype == torch.float64 and my.dtype == torch.float64 and mx.shape == (X.shape[1],) and my.shape == (Y.shape[1],)
        assert mx.is_contiguous() and my.is_contiguous()
        descs[i] = _lib.CkaProduct(_ptr(X), _ptr(mx), X.stride(0), X.shape[1], _ptr(Y), _ptr(my), Y.stride(0), Y.shape[1], X.shape[0])
        dev = X.device
    if out is None:
        out = torch.empty(len(products), dtype=torch.float64, device=dev)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == len(products)
    if not products:
        return out
    lib = _lib.load()
    ws = workspace(dev).get(lib.mafed_cka_hsic_workspace_bytes(descs, len(products)))
    check(lib.mafed_cka_hsic(descs, len(products), _ptr(out), _ptr(ws), ws.numel(), _stream()), "mafed_cka_hsic")
    return out


SELECT_HERDING, SELECT_KCENTER = 0, 1


def select_greedy(X: torch.Tensor, mean: torch.Tensor, mode: int, k: int, want_scores: bool = False):
    """k greedy picks over the rows of X fp32 [n, d] (row stride >= d; read in place) with its fp64 column mean [d] (``cka_stats``):
    herding (``SELECT_HERDING``) or k-center (``SELECT_KCENTER``), the rules of include/mafed_hip.h.
    -> (picks int64 [k], values fp32 [k], last_scores fp32 [n] or None), all on the device; 2 k + 1 launches, no synchronisation."""
    assert X.dtype == torch.float32 and X.dim() == 2 and X.stride(1) == 1
    assert mean.dtype == torch.float64 and mean.shape == (X.shape[1],) and mean.is_contiguous()
    n, d = X.shape
    k = int(k)
    lib = _lib.load()
    picks = torch.empty(max(k, 0), dtype=torch.int64, device=X.device)
    values = torch.empty(max(k, 0), dtype=torch.float32, device=X.device)
    scores = torch.empty(n, dtype=torch.float32, device=X.device) if want_scores else None
    ws = workspace(X.device).get(lib.mafed_select_workspace_bytes(n, d))
    check(lib.mafed_select_greedy(_ptr(X), n, d, X.stride(0), _ptr(mean), int(mode), k, _ptr(picks), _ptr(values), _ptr(scores), _ptr(ws),
                                  ws.numel(), _stream()), "mafed_select_greedy")
    return picks, values, scores


def gradnorm_clip(g: torch.Tensor, max_norm: float, out2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> out[2] = {||g||, clip scale}"""
    _flat_f32(g)
    lib = _lib.load()
    if out2 is None:
        out2 = torch.empty(2, dtype=torch.float32, device=g.device)
    nb = lib.mafed_gradnorm_workspace_bytes(g.numel())
    ws = workspace(g.device).get(nb)
    check(lib.mafed_gradnorm_clip(_ptr(g), g.numel(), float(max_norm), _ptr(out2), _ptr(ws), ws.numel(), _stream()), "mafed_gradnorm_clip")
    return out2


def pad_text_rows(src: torch.Tensor, B: int, S: int, P: int, lp_dtype=None):
    """[B*(S-P), h] fp32 -> ([B*S, h] fp32 with zero image rows, the same in ``lp_dtype`` (bf16) or None)"""
    h = src.shape[-1]
    dst = torch.empty((B * S, h), dtype=torch.float32, device=src.device)
    lp = torch.empty((B * S, h), dtype=lp_dtype, device=src.device) if lp_dtype == torch.bfloat16 else None
    check(_lib.load().mafed_pad_text_rows(_ptr(src), B, S, P, h, _ptr(dst), _ptr(lp), _stream()), "mafed_pad_text_rows")
    return dst, lp


def label_rows(labels: torch.Tensor, Rc: int):
    """labels [B,T] int64 -> (row_of_slot [B*Rc] int32, slot_of_row [B*T] int32, labels_c [B,Rc] int64, overflow [1] int32)"""
    B, T = labels.shape
    dev = labels.device
    ros = torch.empty(B * Rc, dtype=torch.int32, device=dev)
    sor = torch.empty(B * T, dtype=torch.int32, device=dev)
    lc = torch.empty((B, Rc), dtype=torch.int64, device=dev)
    ov = torch.zeros(1, dtype=torch.int32, device=dev)
    check(_lib.load().mafed_label_rows(_ptr(labels), B, T, Rc, _ptr(ros), _ptr(sor), _ptr(lc), _ptr(ov), _stream()), "mafed_label_rows")
    return ros, sor, lc, ov


def pad_text_batch(input_ids: torch.Tensor, attention_mask: torch.Tensor, labels: Optional[torch.Tensor], Tp: int):
    """ids / mask / labels [B,T] int64 (contiguous) -> the same at [B,Tp]: id 0, mask 0, label -100 behind the text.  One launch."""
    B, T = input_ids.shape
    dev = input_ids.device
    out = torch.empty((3 if labels is not None else 2, B, Tp), dtype=torch.int64, device=dev)
    check(_lib.load().mafed_pad_text_batch(_ptr(input_ids), _ptr(attention_mask), _ptr(labels), B, T, int(Tp), _ptr(out[0]), _ptr(out[1]),
                                           _ptr(out[2]) if labels is not None else 0, _stream()), "mafed_pad_text_batch")
    return out[0], out[1], (out[2] if labels is not None else None)


def gemm_fallback_launches() -> int:
    """bf16 GEMM launches that reached the register-staged kernel so far (shapes that tile none of the fast kernels)."""
    return int(_lib.load().mafed_gemm_fallback_launches())


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """dst[r] = src[idx[r]] (zeros where idx[r] < 0); src [n,h] contiguous fp32 / bf16, idx int32"""
    h = src.shape[-1]
    dst = torch.empty((idx.numel(), h), dtype=src.dtype, device=src.device)
    check(_lib.load().mafed_gather_rows(_ptr(src), _dt(src), _ptr(idx), idx.numel(), h, _ptr(dst), _stream()), "mafed_gather_rows")
    return dst


def gradnorm_blocks(n: int) -> int:
    return int(_lib.load().mafed_gradnorm_blocks(int(n)))


def gradnorm_partial(g: torch.Tensor, partial_out: torch.Tensor) -> None:
    """sum-of-squares partials of the (contiguous, 16-byte aligned) range ``g`` -> partial_out[:gradnorm_blocks(g.numel())]"""
    _flat_f32(g)
    check(_lib.load().mafed_gradnorm_partial(_ptr(g), g.numel(), _ptr(partial_out), _stream()), "mafed_gradnorm_partial")


def gradnorm_finish(partials: torch.Tensor, max_norm: float, out2: torch.Tensor, advance=None, norm_log: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fold the per-range partials into out2 = {norm, clip scale}.  ``advance`` = (state, base_lr, warmup, total, beta1, beta2, hyper):
    the optimiser's schedule advance rides in the same launch (mafed_gradnorm_finish_advance); ``norm_log`` = a 1-element slot that
    also receives the norm."""
    if advance is None:
        check(_lib.load().mafed_gradnorm_finish(_ptr(partials), partials.numel(), float(max_norm), _ptr(out2), _stream()), "mafed_gradnorm_finish")
        if norm_log is not None:
            norm_log.copy_(out2[0:1])
    else:
        state, base_lr, warmup, total, b1, b2, hyper = advance
        check(_lib.load().mafed_gradnorm_finish_advance(_ptr(partials), partials.numel(), float(max_norm), _ptr(out2), _ptr(norm_log), _ptr(state),
                                                        float(base_lr), int(warmup), int(total), float(b1), float(b2), _ptr(hyper), _stream()),
              "mafed_gradnorm_finish_advance")
    return out2


def adamw_step_(p, g, m, v, lr_dev, beta1, beta2, eps, weight_decay, step, clip=None, grad_mul=1.0, p_bf16=None, zero_grad: bool = False,
                zero_n: Optional[int] = None) -> None:
    """``zero_grad``: the kernel also writes zeros over ``g`` (the next window's optimizer.zero_grad(), same pass); ``zero_n``: only over
    its first ``zero_n`` elements (mafed_adamw_step_partial_zero: the rest is overwritten by the next window's weight-gradient GEMMs)."""
    if zero_grad and zero_n is not None and zero_n < p.numel():
        check(_lib.load().mafed_adamw_step_partial_zero(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(lr_dev), beta1, beta2, eps, weight_decay,
                                                        int(step), _ptr(clip), float(grad_mul), _ptr(p_bf16), int(zero_n), _stream()), "mafed_adamw_step")
        return
    fn = _lib.load().mafed_adamw_step_zero_grad if zero_grad else _lib.load().mafed_adamw_step
    check(fn(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(lr_dev), beta1, beta2, eps, weight_decay,
             int(step), _ptr(clip), float(grad_mul), _ptr(p_bf16), _stream()), "mafed_adamw_step")


def adam_family_step_(rule: str, p, g, m, s, lr_dev, beta1, beta2, eps, weight_decay, step, clip=None, grad_mul=1.0, p_bf16=None,
                      zero_n: int = 0) -> None:
    """torch.optim.Adam (``rule="adam"``, ``s`` = exp_avg_sq) or Adamax (``rule="adamax"``, ``s`` = exp_inf) on one flat segment, same
    conventions as ``adamw_step_``; ``zero_n``: the first ``zero_n`` elements of ``g`` are zeroed in the same pass (0 = none, numel = all)."""
    fn = {"adam": "mafed_adam_step", "adamax": "mafed_adamax_step"}[rule]
    check(getattr(_lib.load(), fn)(_ptr(p), _ptr(g), _ptr(m), _ptr(s), p.numel(), _ptr(lr_dev), float(beta1), float(beta2), eps, weight_decay, int(step),
                                   _ptr(clip), float(grad_mul), _ptr(p_bf16), int(zero_n), _stream()), fn)


def optim_advance_(state: torch.Tensor, base_lr: float, warmup: int, total: int, beta1: float, beta2: float, hyper: torch.Tensor,
                   clip: Optional[torch.Tensor] = None) -> None:
    """``clip`` = the {norm, scale} pair of this step's clip: a skipped step (scale < 0: non-finite norm) does not advance the counter."""
    check(_lib.load().mafed_optim_advance_guarded(_ptr(state), float(base_lr), int(warmup), int(total), float(beta1), float(beta2),
                                                  _ptr(hyper), _ptr(clip), _stream()), "mafed_optim_advance")


def cast(src: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert src.is_contiguous()
    if out is None:
        out = torch.empty(src.shape, dtype=dtype, device=src.device)
    check(_lib.load().mafed_cast(_ptr(src), _dt(src), _ptr(out), _dt(out), src.numel(), _stream()), "mafed_cast")
    return out


def gelu(x: torch.Tensor) -> torch.Tensor:
    y = torch.empty_like(x)
    check(_lib.load().mafed_gelu(_ptr(x), _ptr(y), _dt(x), x.numel(), _stream()), "mafed_gelu")
    return y
