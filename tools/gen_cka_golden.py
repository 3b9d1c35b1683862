"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/cka.npz from the reference's own feature_space_linear_cka (mafed/analysis/cka.py),
biased and debiased, in float64 numpy on the CPU.  Needs the reference checkout on PYTHONPATH, as oracle/gen_golden.py does:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/gen_cka_golden.py

Every case stores its fp32 inputs (case/<name>/x, /y) and the two CKA values (/cka, /cka_debiased) computed on those fp32 values
widened to float64.
"""
import os

import numpy as np
from mafed.analysis.cka import feature_space_linear_cka

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cka.npz")


def cases():
    rng = np.random.default_rng(1234)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)   # noqa: E731
    out = {}
    out["n_lt_h"] = (f(40, 100), f(40, 100))                     # n < h
    x = f(300, 64)
    out["n_gt_h"] = (x, (x @ f(64, 64) * 0.3 + f(300, 64)).astype(np.float32))   # n > h, related
    out["hx_ne_hy"] = (f(200, 96), f(200, 40))                   # hx != hy
    out["odd_n5_h100"] = (f(5, 100), f(5, 100))                  # odd sizes
    spread = np.exp(rng.uniform(-1, 2, size=(1, 128))).astype(np.float32)
    x = f(257, 128) * spread
    off = (1e3 * spread * rng.choice([-1.0, 1.0], size=(1, 128))).astype(np.float32)
    out["offset_1e3"] = ((x + off).astype(np.float32), (x @ f(128, 128) * 0.1 + x + off).astype(np.float32))   # columns offset by 1e3 x spread
    x = f(300, 96)
    out["near_identical"] = (x, (x + 0.03 * f(300, 96)).astype(np.float32))   # CKA ~ 0.999
    out["unrelated"] = (f(500, 64), f(500, 64))
    return out


def main():
    arrays = {}
    for name, (x, y) in cases().items():
        xd, yd = x.astype(np.float64), y.astype(np.float64)
        arrays[f"case/{name}/x"] = x
        arrays[f"case/{name}/y"] = y
        arrays[f"case/{name}/cka"] = np.float64(feature_space_linear_cka(xd, yd))
        arrays[f"case/{name}/cka_debiased"] = np.float64(feature_space_linear_cka(xd, yd, debiased=True))
        print(f"{name:16s} n={x.shape[0]:5d} hx={x.shape[1]:4d} hy={y.shape[1]:4d}  cka {float(arrays[f'case/{name}/cka']):.9f}  "
              f"debiased {float(arrays[f'case/{name}/cka_debiased']):.9f}")
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
