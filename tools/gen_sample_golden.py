"""Golden sampling fixture (tests/golden/sample.npz) for the token sampler (csrc/sample.hip) and ``model.sample``.  Authoring only, CPU.

Kernel cases: two logit recipes (tests/sample_ref.py::case_logits) at V in {512, 50 277, 50 304}, R = 5, under eight parameter sets.  The
logits are regenerated from the stored seed (a checksum guards the recipe); stored are the kept masks (bit-packed), the uniforms and the
expected tokens.  The masks come from transformers' own Temperature / TopK / TopP / MinP warpers in HF's order; the tokens from an fp64
inverse CDF in ascending id.  Where an exact tie sits on the top-p cut the warper keeps an order-dependent part of the tie and the
sampler keeps all of it (its one documented deviation): the stored mask is then the warper's completed with the tied ids, and the
generator asserts that nothing else differs.  A seed is accepted only if no threshold decision of any row lies within the case's margin
of its cut (sample_ref.case_margin: 5e-4; mass against top_p, relative probability against min_p), so neither side's rounding decides.

End-to-end cases: the sampling loop around ``oracle.vlpythia_ref.forward`` on the growing sequence, inputs expanded n times, uniforms
from the numpy Philox of (seed, row, step).  A seed is accepted only if at every step of every live row u stays >= 1e-3 away from the
nearest CDF edge and the kept set's decisions keep a margin of 2e-3 (top-k: the k-th and (k+1)-th z are >= 5e-3 apart): the fp32
engine's logits differ from the oracle's by about 1e-5.

    python tools/gen_sample_golden.py          # rewrites tests/golden/sample.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import vlpythia_ref as R  # noqa: E402
from tests import sample_ref as S  # noqa: E402
from tests.helpers import TINY, tiny_cfg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sample.npz")
SEED = 131

# tiny config -> (temperature, top_k, top_p, min_p): random weights give nearly flat logits, so the temperatures are low
E2E_WARP = {"t64": (0.05, 8, 1.0, 0.0), "m64": (0.04, 0, 1.0, 0.1), "t128": (0.05, 12, 0.9, 0.0)}
E2E_MAX_NEW = 5
E2E_CASES = {f"{name}_n{n}{'_eos' if eos else ''}": (name, n, eos) for name in ("t64", "m64", "t128") for n in (1, 3) for eos in (False, True)}
EDGE = 1e-3
TOPK_GAP = 5e-3
E2E_MARGIN = 2e-3   # the low temperatures multiply the engine's 1e-5 logit error by 20 .. 25 on its way into z


# ---- kernel cases ----------------------------------------------------------------------------------------------------------------
def kernel_case(recipe, V, s, seed):
    """-> dict of the stored arrays, or None when the seed leaves a decision too close to its cut."""
    T, k, p, mp = S.PARAM_SETS[s]
    logits = S.case_logits(recipe, V, seed)
    mask, margin = S.kept_by_value(logits, T, k, p, mp)
    if float(margin.min()) < S.case_margin(recipe, V, s):
        return None
    hf = S.hf_mask(logits, T, k, p, mp).numpy()
    z = logits.double().numpy() / T
    for r in range(S.ROWS):
        diff = mask[r] != hf[r]
        if diff.any():   # only the tie on the top-p cut: ids the warper dropped that share the smallest kept value
            assert p < 1.0 and not (hf[r] & ~mask[r]).any(), (recipe, V, s, r)
            assert np.all(z[r][diff] == z[r][hf[r]].min()), (recipe, V, s, r)
    u = np.random.RandomState(seed + 7).rand(S.ROWS).astype(np.float32)
    tokens = np.array([S.draw(S.cdf(logits[r].numpy(), T, mask[r])[1], mask[r], float(u[r])) for r in range(S.ROWS)], dtype=np.int64)
    return dict(seed=np.int64(seed), checksum=np.float64(logits.double().abs().sum()), mask=S.pack_mask(mask), hf_differs=np.int64((mask != hf).sum()),
                margin=margin, uniforms=u, tokens=tokens)


# ---- end-to-end cases ---------------------------------------------------------------------------------------------------------------
def e2e_inputs(case):
    name, n, eos = E2E_CASES[case]
    cfg, t = tiny_cfg(name), TINY[name]
    sd = R.init_weights(cfg, seed=SEED)
    batch = R.make_batch(cfg, t["B"], t["T"], seed=SEED + 1, pad=True)
    return cfg, sd, batch, n, E2E_WARP[name]


def oracle_logits(sd, cfg, feats, ids, am):
    with torch.no_grad():
        return R.forward(sd, {"input_ids": ids, "attention_mask": am, "patch_embeddings": feats}, cfg).logits[:, -1, :].float()


def sample_loop(cfg, sd, batch, n, warp, seed, eos, max_new):
    """-> (tokens [R, max_new], uniforms [max_new, R], edge distance [max_new, R], logprobs [R, max_new], smallest decision margin, 0 when a top-k boundary is a
    near-tie: the k-th and (k+1)-th z less than TOPK_GAP apart)."""
    T, k, p, mp = warp
    ids = batch["input_ids"].repeat_interleave(n, 0)
    am = batch["attention_mask"].repeat_interleave(n, 0)
    feats = batch["patch_embeddings"].repeat_interleave(n, 0)
    rows = ids.shape[0]
    unfinished = np.ones(rows, dtype=bool)
    toks, us, edges, lps, worst, topk_clear = [], [], [], [], np.inf, True
    for t in range(max_new):
        lg = oracle_logits(sd, cfg, feats, ids, am)
        u = S.uniforms(seed, rows, t)
        mask, margin = S.kept_by_value(lg, T, k, p, mp)
        z = lg.double().numpy() / T
        nxt, edge, lp = np.zeros(rows, dtype=np.int64), np.full(rows, np.inf), np.zeros(rows)
        for r in range(rows):
            if not unfinished[r]:
                nxt[r] = eos
                continue
            worst = min(worst, float(margin[r]))
            if 0 < k < z.shape[1]:
                zs = np.sort(z[r])
                topk_clear = topk_clear and float(zs[-k] - zs[-k - 1]) >= TOPK_GAP
            prob, cum = S.cdf(lg[r].numpy(), T, mask[r])
            nxt[r] = S.draw(cum, mask[r], u[r])
            edge[r] = float(np.abs(cum[mask[r]] - u[r]).min())
            edge[r] = min(edge[r], u[r])   # (the CDF's lower end)
            lp[r] = np.log(prob[nxt[r]])
            if eos is not None and nxt[r] == eos:
                unfinished[r] = False
        toks.append(nxt), us.append(u), edges.append(edge), lps.append(lp)
        ids = torch.cat([ids, torch.from_numpy(nxt)[:, None]], 1)
        am = torch.cat([am, torch.ones(rows, 1, dtype=am.dtype)], 1)
    return np.stack(toks, 1), np.stack(us), np.stack(edges), np.stack(lps, 1), (worst if topk_clear else 0.0)


def e2e_case(case):
    name, n, want_eos = E2E_CASES[case]
    cfg, sd, batch, n, warp = e2e_inputs(case)
    for seed in range(1000 + 17 * len(case), 1000 + 17 * len(case) + 400):
        eos = None
        if want_eos:   # the token row 0 draws at its third step without an eos: with random weights no fixed id is ever likely
            eos = int(sample_loop(cfg, sd, batch, n, warp, seed, None, 3)[0][0, 2])
        toks, us, edges, lps, worst = sample_loop(cfg, sd, batch, n, warp, seed, eos, E2E_MAX_NEW)
        if float(edges.min()) >= EDGE and worst >= E2E_MARGIN:
            if eos is not None:   # cut like the engine: at the slowest row's first eos
                first = [(list(row).index(eos) + 1) if eos in row else len(row) for row in toks]
                toks, lps = toks[:, :max(first)], lps[:, :max(first)]
            return dict(seed=np.int64(seed), eos=np.int64(-1 if eos is None else eos), tokens=toks, uniforms=us, edge=edges,
                        logprobs=lps.astype(np.float32), margin=np.float64(worst))
    raise RuntimeError(f"{case}: no seed keeps every draw {EDGE} away from a CDF edge")


def main():
    out = {}
    for recipe in S.RECIPES:
        for V in S.VOCABS:
            for s in range(len(S.PARAM_SETS)):
                base = 10000 * (1 + S.RECIPES.index(recipe)) + 100 * s + V % 97
                for seed in range(base, base + 20000000, 1000):
                    c = kernel_case(recipe, V, s, seed)
                    if c is not None:
                        break
                else:
                    raise RuntimeError(f"{recipe} V={V} set {s}: no seed meets the margin")
                for key, v in c.items():
                    out[f"k/{recipe}/{V}/{s}/{key}"] = v
                print(f"kernel case {recipe} V={V} set {s} {S.PARAM_SETS[s]}: seed {seed}, kept {S.unpack_mask(c['mask'], V).sum(1).tolist()}, "
                      f"margin {float(c['margin'].min()):.2e}, ids outside the warper's mask {int(c['hf_differs'])}", flush=True)
    for case in E2E_CASES:
        c = e2e_case(case)
        for key, v in c.items():
            out[f"e/{case}/{key}"] = v
        print(f"end-to-end case {case}: seed {int(c['seed'])} eos {int(c['eos'])} tokens {c['tokens'].tolist()} min edge {float(c['edge'].min()):.2e}", flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
