"""Throughput of the CKA analysis kernels (csrc/cka.hip) on the GPU, against the in-tree fp32 GEMM path and the reference's float64 numpy.

    python tools/cka_bench.py [--quick] [--out FILE]

Legs (every timed window warmed up first, device-synchronised, best of --reps):
  pool      modality pooling at 410M (L = 24, h = 1024), B = 32, 256 image + 32 text rows: bytes read + written / time vs 8 TB/s HBM
  hsic      batches of 2L = 48 cross products (X_p, Y_p distinct sets drawn from a pool of 8 [n, h] sets) at n in {8192, 32768, 131072},
            h in {1024, 2048}: algorithmic FLOP (2 n h^2 per cross term) / time vs the 157.3 TF fp32 matrix peak
  hsic_sym  the same sets as 48 self terms (n h^2 each: upper-triangle tiles only)
  gemm      the same cross products through ops.gemm (the exact fp32 VALU parity kernel) on pre-centred fp32 copies + a sum of squares
  numpy     float64 numpy of feature_space_linear_cka (cka.py:116-175) for one pair at n = 32768, h = 1024 (the reference's path)
  run       one whole 410M run: 5 checkpoints x 48 feature sets at n = 32768 through modality_cka, end to end
Kernel times for the same legs come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--quick).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mafed_amd import ops  # noqa: E402
from mafed_amd.analysis import modality_cka  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12
DEV = "cuda"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def log(fp, s):
    print(s, flush=True)
    fp.write(s + "\n")
    fp.flush()


def bench_pool(fp, reps):
    L, B, P, T, h = 24, 32, 256, 32, 1024
    S = P + T
    g = torch.Generator(device=DEV).manual_seed(1)
    hs = [torch.randn(B, S, h, device=DEV, generator=g) for _ in range(L)]
    mask = torch.ones(B, T, dtype=torch.int64, device=DEV)
    out = torch.empty(2, L, B, h, device=DEV)
    t = timed(lambda: ops.cka_pool(hs, mask, P, out), reps)
    nbytes = 4.0 * L * B * (P + T) * h + 4.0 * 2 * L * B * h
    log(fp, f"pool   L={L} B={B} P+T={P}+{T} h={h}: {t * 1e6:9.1f} us  {nbytes / t / 1e12:6.2f} TB/s  ({nbytes / t / PEAK_HBM:5.1%} of HBM peak, call time)")


def bench_hsic(fp, n, h, reps, with_gemm):
    nsets, G = 8, 48
    g = torch.Generator(device=DEV).manual_seed(n + h)
    sets = [torch.randn(n, h, device=DEV, generator=g) + 3.0 for _ in range(nsets)]
    means = [ops.cka_stats(s, row_norms=False)[0][0] for s in sets]
    cross = [(sets[i % nsets], means[i % nsets], sets[(i + 1 + i // nsets) % nsets], means[(i + 1 + i // nsets) % nsets]) for i in range(G)]
    selfp = [(sets[i % nsets], means[i % nsets], sets[i % nsets], means[i % nsets]) for i in range(G)]
    out = torch.empty(G, dtype=torch.float64, device=DEV)
    fl = 2.0 * n * h * h * G
    t = timed(lambda: ops.cka_hsic(cross, out=out), reps)
    ref = out.clone()
    log(fp, f"hsic     n={n:6d} h={h} G={G}: {t * 1e3:9.2f} ms  {fl / t / 1e12:6.1f} TF  ({fl / t / PEAK_F32_MATRIX:5.1%} of fp32 matrix peak, call time)")
    ts = timed(lambda: ops.cka_hsic(selfp, out=out), reps)
    fls = 1.0 * n * h * h * G
    log(fp, f"hsic_sym n={n:6d} h={h} G={G}: {ts * 1e3:9.2f} ms  {fls / ts / 1e12:6.1f} TF  ({fls / ts / PEAK_F32_MATRIX:5.1%} of fp32 matrix peak, call time)")
    if not with_gemm:
        return
    cen = [(s - m.float()).contiguous() for s, m in zip(sets, means)]
    cpairs = [(cen[i % nsets], cen[(i + 1 + i // nsets) % nsets]) for i in range(G)]
    C = torch.empty(h, h, device=DEV)
    acc = torch.empty(G, dtype=torch.float64, device=DEV)

    def gemm_path():
        for i, (a, b) in enumerate(cpairs):
            ops.gemm(a, b, True, False, out=C)
            acc[i] = C.double().square().sum()
    tg = timed(gemm_path, max(1, reps // 2))
    rel = float(((acc - ref).abs() / ref).max())
    log(fp, f"gemm     n={n:6d} h={h} G={G}: {tg * 1e3:9.2f} ms  {fl / tg / 1e12:6.1f} TF  (ops.gemm fp32 + sum of squares; hsic is "
            f"{tg / t:4.2f}x faster; max rel diff {rel:.1e})")
    del cen, cpairs


def bench_numpy(fp, n=32768, h=1024):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, h))
    y = 0.5 * x + rng.standard_normal((n, h))

    def ref_cka(features_x, features_y):   # cka.py:116-138 (biased), float64
        features_x = features_x - np.mean(features_x, 0, keepdims=True)
        features_y = features_y - np.mean(features_y, 0, keepdims=True)
        dot_product_similarity = np.linalg.norm(features_x.T.dot(features_y)) ** 2
        normalization_x = np.linalg.norm(features_x.T.dot(features_x))
        normalization_y = np.linalg.norm(features_y.T.dot(features_y))
        return dot_product_similarity / (normalization_x * normalization_y)
    t0 = time.perf_counter()
    ref_cka(x, y)
    t = time.perf_counter() - t0
    fl = 2.0 * n * h * h * 3
    log(fp, f"numpy    n={n:6d} h={h} one pair: {t * 1e3:9.1f} ms  {fl / t / 1e9:6.1f} GFLOP/s float64 (reference's path, "
            f"{os.environ.get('OMP_NUM_THREADS', '?')} threads)")
    return t


def bench_run(fp, n=32768, reps=2):
    K, L, h = 5, 24, 1024
    g = torch.Generator(device=DEV).manual_seed(5)
    base = torch.randn(2, L, n, h, device=DEV, generator=g)
    feats = [base + 0.3 * k * torch.randn(2, L, n, h, device=DEV, generator=g) for k in range(K)]
    t = timed(lambda: modality_cka(feats, reference=0), reps)
    fl = K * 2 * L * 1.0 * n * h * h + (K - 1) * 2 * L * 2.0 * n * h * h
    log(fp, f"run      410M: {K} checkpoints x {2 * L} sets, n={n}: {t * 1e3:9.1f} ms end to end  ({fl / t / 1e12:5.1f} TF algorithmic incl. "
            f"statistics and host work)")
    del feats, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one HSIC shape per width, no GEMM / numpy legs (for the profiler run)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fp = open(a.out, "a") if a.out else open(os.devnull, "w")
    assert torch.cuda.is_available(), "cka_bench needs a GPU"
    bench_pool(fp, a.reps)
    shapes = [(32768, 1024), (32768, 2048)] if a.quick else [(n, h) for h in (1024, 2048) for n in (8192, 32768, 131072)]
    for n, h in shapes:
        bench_hsic(fp, n, h, a.reps, with_gemm=not a.quick)
        torch.cuda.empty_cache()
    if not a.quick:
        bench_run(fp)
        bench_numpy(fp)
    fp.close()


if __name__ == "__main__":
    main()
