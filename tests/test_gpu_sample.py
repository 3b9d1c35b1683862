"""GPU: the token sampler (``ops.sample_token``, csrc/sample.hip) against transformers' warpers and an fp64 inverse CDF
(tests/golden/sample.npz, tools/gen_sample_golden.py, tests/sample_ref.py), and ``model.sample`` end to end: recompute, cached, n
samples over one prefill, replayed from a hipGraph."""
import functools

import numpy as np
import pytest
import torch

from tests import sample_ref as S
from tests.helpers import load_golden
from tests.test_gpu_model import DEV, build_model, close, to_dev
from tools import gen_sample_golden as G

pytestmark = pytest.mark.gpu

# |CDF of the kernel - fp64 CDF|: a sum of <= 65 536 non-negative terms in any fixed tree of fp32 adds is off by <= 17 * 2^-24 of the
# total, exp by <= 2 ulp = 2^-22 (the kernel's integer masses are tighter than either): 17 * 2^-24 + 2^-22 < 4e-6.
CDF_TOL = 4e-6


@functools.lru_cache(maxsize=4)
def _logits(recipe, V, seed):
    return S.case_logits(recipe, V, seed)


def _kcase(recipe, V, s):
    g = load_golden("sample.npz")
    pre = f"k/{recipe}/{V}/{s}/"
    return (_logits(recipe, V, int(g[pre + "seed"])), S.PARAM_SETS[s], S.unpack_mask(g[pre + "mask"], V), g[pre + "uniforms"], g[pre + "tokens"])


def _run(logits_dev, warp, u, want_kept=True, want_lp=False, **kw):
    from mafed_amd import ops
    R = logits_dev.shape[0]
    kept = torch.zeros(R, dtype=torch.int32, device=DEV) if want_kept else None
    lp = torch.zeros(R, dtype=torch.float32, device=DEV) if want_lp else None
    un = None if u is None else torch.as_tensor(np.asarray(u, dtype=np.float32)).to(DEV)
    tok = ops.sample_token(logits_dev, *warp, uniforms=un, kept=kept, logprob=lp, **kw)
    return tok.cpu().numpy(), None if kept is None else kept.cpu().numpy(), None if lp is None else lp.cpu().numpy()


def _assert_draws(logits, T, mask, tok, u, rows, what):
    """Every drawn id is kept and its fp64 CDF interval, widened by CDF_TOL, holds u (rows[i]: the fixture row behind draw i)."""
    for r in sorted(set(rows.tolist())):
        p, cum = S.cdf(logits[r].numpy(), T, mask[r])
        sel = rows == r
        t, uu = tok[sel], np.asarray(u, dtype=np.float64)[sel]
        assert mask[r][t].all(), f"{what} row {r}: a drawn id is outside the kept set"
        lo, hi = cum[t] - p[t], cum[t]
        worst = float(np.maximum(lo - uu, uu - hi).max())
        print(f"[sample] {what} row {r}: {int(sel.sum())} draws, worst distance outside the fp64 interval {worst:.3e} (bound {CDF_TOL:.1e})")
        assert worst <= CDF_TOL, f"{what} row {r}: u outside the drawn id's interval by {worst:.3e}"


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", S.VOCABS)
def test_kept_set_equals_the_warpers(V, dt):
    """1: the kept-set size is the fixture mask's and the fixture's uniforms draw ids of that mask, for both recipes and all eight sets."""
    for recipe in S.RECIPES:
        for s in range(len(S.PARAM_SETS)):
            logits, warp, mask, u, tokens = _kcase(recipe, V, s)
            tok, kept, _ = _run(logits.to(dt).to(DEV), warp, u)
            assert np.array_equal(kept, mask.sum(1)), (recipe, s, kept, mask.sum(1))
            _assert_draws(logits, warp[0], mask, tok, u, np.arange(S.ROWS), f"{recipe} V={V} set {s}")
            edge = np.array([np.abs(S.cdf(logits[r].numpy(), warp[0], mask[r])[1] - float(u[r])).min() for r in range(S.ROWS)])
            sure = edge > CDF_TOL   # u is not within the bound of a CDF edge: the id is the fp64 one
            assert np.array_equal(tok[sure], tokens[sure]), (recipe, s)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", S.VOCABS)
def test_every_kept_token_is_reachable_and_only_those(V, dt):
    """2: small kept sets (<= 64 ids): the fp64 midpoint of every kept id's CDF interval returns exactly that id.  Larger ones: 64
    uniforms per row over (0, 1) return kept ids whose interval, widened by the derived bound, holds u."""
    rs = np.random.RandomState(V)
    for recipe in S.RECIPES:
        for s in range(len(S.PARAM_SETS)):
            logits, warp, mask, _, _ = _kcase(recipe, V, s)
            counts = mask.sum(1)
            if int(counts.max()) <= 64:
                dev = logits.to(dt).to(DEV)
                cdfs = [S.cdf(logits[r].numpy(), warp[0], mask[r]) for r in range(S.ROWS)]
                ids = [np.nonzero(mask[r])[0] for r in range(S.ROWS)]
                for j in range(int(counts.max())):
                    want = np.array([ids[r][min(j, len(ids[r]) - 1)] for r in range(S.ROWS)])
                    u = np.array([cdfs[r][1][want[r]] - 0.5 * cdfs[r][0][want[r]] for r in range(S.ROWS)])
                    tok, _, _ = _run(dev, warp, u, want_kept=False)
                    assert np.array_equal(tok, want), (recipe, s, j, tok, want)
            else:
                big = logits.to(dt).to(DEV).repeat(64, 1)   # draw i uses fixture row i % ROWS
                u = rs.rand(64 * S.ROWS).astype(np.float32).clip(1e-7, 1 - 1e-7)
                tok, _, _ = _run(big, warp, u, want_kept=False)
                _assert_draws(logits, warp[0], mask, tok, u, np.arange(64 * S.ROWS) % S.ROWS, f"{recipe} V={V} set {s} {dt}")


@pytest.mark.parametrize("recipe,s", [("flat", 0), ("flat", 3), ("flat", 5), ("planted", 0)])
def test_large_kept_sets_id_by_id(recipe, s):
    """1 / 2, dense: at V = 512 every kept id of a LARGE kept set is drawn by the fp64 midpoint of its CDF interval, where that interval
    is wider than twice the bound (one launch of rows x 512 draws; an id outside the mask, or a kept id that cannot be reached, fails)."""
    V = 512
    logits, warp, mask, _, _ = _kcase(recipe, V, s)
    dev = logits.to(DEV).repeat(V, 1)   # draw i: fixture row i % ROWS, target the (i // ROWS)-th id
    want = np.zeros(V * S.ROWS, dtype=np.int64)
    u = np.zeros(V * S.ROWS)
    wide = np.zeros(V * S.ROWS, dtype=bool)
    for r in range(S.ROWS):
        p, cum = S.cdf(logits[r].numpy(), warp[0], mask[r])
        ids = np.nonzero(mask[r])[0]
        tgt = ids[np.minimum(np.arange(V), len(ids) - 1)]
        want[r::S.ROWS], u[r::S.ROWS], wide[r::S.ROWS] = tgt, cum[tgt] - 0.5 * p[tgt], (p[tgt] > 4 * CDF_TOL) & (np.arange(V) < len(ids))
    tok, kept, _ = _run(dev, warp, u)
    assert np.array_equal(kept, np.tile(mask.sum(1), V))
    assert all(mask[i % S.ROWS][tok[i]] for i in range(V * S.ROWS))
    print(f"[sample] {recipe} set {s}: {int(wide.sum())} of {int(sum(mask.sum(1)))} kept ids have an interval wide enough to be hit by its midpoint")
    assert wide.sum() >= 0.5 * mask.sum() or recipe == "planted"
    assert np.array_equal(tok[wide], want[wide])


@pytest.mark.parametrize("V", S.VOCABS)
def test_top_k_one_is_the_argmax(V):
    """3: for any u and temperature (rows without ties: the planted recipe's top id stands alone)."""
    logits = _kcase("planted", V, 7)[0]
    want = logits.argmax(-1).numpy()
    for dt in (torch.float32, torch.bfloat16):
        dev = logits.to(dt).to(DEV)
        for T in (0.3, 1.0, 2.5):
            for u in (1e-7, 0.5, 1 - 1e-7):
                tok, kept, _ = _run(dev, (T, 1, 1.0, 0.0), np.full(S.ROWS, u))
                assert np.array_equal(tok, want) and np.array_equal(kept, np.ones(S.ROWS))


def test_generated_uniforms_are_philox_of_seed_row_and_step():
    """4: uniforms=None draws with Philox4x32-10 of (seed, row, step); a row's number does not depend on R."""
    from mafed_amd import ops
    logits = torch.randn(7, 50277, generator=torch.Generator().manual_seed(4)).to(DEV)
    warp = (0.9, 0, 1.0, 0.0)
    for seed in (1234567, 0xfedcba9876543210):
        word = ops.seed_word(seed, DEV)
        for step in (0, 5):
            got7 = ops.sample_token(logits, *warp, seed=word, step=step).cpu().numpy()
            want7, _, _ = _run(logits, warp, S.uniforms(seed, 7, step), want_kept=False)
            assert np.array_equal(got7, want7), (seed, step)
            got3 = ops.sample_token(logits[:3], *warp, seed=word, step=step).cpu().numpy()
            assert np.array_equal(got3, got7[:3])
        assert not np.array_equal(ops.sample_token(logits, *warp, seed=word, step=0).cpu().numpy(),
                                  ops.sample_token(logits, *warp, seed=word, step=5).cpu().numpy())


@pytest.mark.parametrize("V", S.VOCABS)
def test_same_bits_on_every_run_and_logprob_within_fp64(V):
    """5: token and logprob are bitwise the same from run to run; the logprob is within 1e-5 of fp64."""
    for recipe, s in (("planted", 4), ("flat", 3), ("flat", 0), ("planted", 6)):
        logits, warp, mask, u, _ = _kcase(recipe, V, s)
        for dt in (torch.float32, torch.bfloat16):
            dev = logits.to(dt).to(DEV)
            runs = [_run(dev, warp, u, want_lp=True) for _ in range(3)]
            for tok, _, lp in runs[1:]:
                assert np.array_equal(tok, runs[0][0]) and np.array_equal(lp.view(np.int32), runs[0][2].view(np.int32))
            tok, _, lp = runs[0]
            want = np.array([np.log(S.cdf(logits[r].numpy(), warp[0], mask[r])[0][tok[r]]) for r in range(S.ROWS)])
            err = float(np.abs(lp - want).max())
            print(f"[sample] logprob {recipe} V={V} set {s} {dt}: max |err| {err:.3e} (bound 1e-5)")
            assert err <= 1e-5


def test_finished_rows_emit_pad_and_a_drawn_eos_clears_the_flag():
    """6."""
    logits, warp, mask, u, tokens = _kcase("planted", 512, 2)
    dev = logits.to(DEV)
    tok0, _, _ = _run(dev, warp, u, want_kept=False)
    eos, pad = int(tok0[1]), 499
    unfinished = torch.tensor([1, 1, 0, 1, 0], dtype=torch.int64, device=DEV)
    tok, kept, lp = _run(dev, warp, u, want_lp=True, unfinished=unfinished, eos_token_id=eos, pad_token_id=pad)
    assert tok[2] == pad and tok[4] == pad and kept[2] == 0 and lp[4] == 0.0
    assert np.array_equal(tok[[0, 1, 3]], tok0[[0, 1, 3]])
    want = np.array([1, 1, 0, 1, 0]) * (tok != eos)
    assert want[1] == 0 and np.array_equal(unfinished.cpu().numpy(), want)
    # no eos: the flags stay
    unfinished = torch.ones(5, dtype=torch.int64, device=DEV)
    _run(dev, warp, u, unfinished=unfinished)
    assert int(unfinished.sum()) == 5


def _e2e(case):
    g = load_golden("sample.npz")
    cfg, sd, batch, n, warp = G.e2e_inputs(case)
    eos = int(g[f"e/{case}/eos"])
    return (cfg, sd, batch, n, warp, None if eos < 0 else eos, int(g[f"e/{case}/seed"]), torch.from_numpy(g[f"e/{case}/tokens"]),
            g[f"e/{case}/logprobs"], g[f"e/{case}/edge"])


def _sample(model, b, n, warp, eos, seed, dtype=None, **kw):
    pe = b["patch_embeddings"] if dtype is None else b["patch_embeddings"].to(dtype)
    return model.sample(input_ids=b["input_ids"], attention_mask=b["attention_mask"], patch_embeddings=pe, max_new_tokens=G.E2E_MAX_NEW,
                        eos_token_id=eos, pad_token_id=eos, temperature=warp[0], top_k=warp[1], top_p=warp[2], min_p=warp[3],
                        num_return_sequences=n, seed=seed, **kw)


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("case", list(G.E2E_CASES))
def test_sample_fp32_matches_the_oracle_loop(case, use_cache):
    """7: recompute, cached (n = 1) and shared-prefix (n = 3) paths all give the fixture's tokens, hence each other's."""
    cfg, sd, batch, n, warp, eos, seed, tokens, logprobs, edge = _e2e(case)
    model = build_model(cfg, sd)
    b = to_dev(batch)
    out, lp = _sample(model, b, n, warp, eos, seed, use_cache=use_cache, return_logprobs=True)
    T = b["input_ids"].shape[1]
    assert out.shape == (tokens.shape[0], T + tokens.shape[1]), (out.shape, tokens.shape)
    assert torch.equal(out[:, :T].cpu(), batch["input_ids"].repeat_interleave(n, 0))
    assert torch.equal(out[:, T:].cpu(), tokens), (out[:, T:].cpu(), tokens)
    close(lp, logprobs, 1e-4, "log-probabilities of the drawn tokens")


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("case", ["t64_n1_eos", "t128_n3_eos"])
def test_sample_step_logits_and_logprobs_share_the_eos_cut(case, use_cache):
    """7b: with an eos, step logits and log-probabilities asked for together: both are cut where the sequences are, and stay in step with them."""
    cfg, sd, batch, n, warp, eos, seed, tokens, logprobs, edge = _e2e(case)
    assert eos is not None
    model = build_model(cfg, sd)
    b = to_dev(batch)
    out, steps, lp = _sample(model, b, n, warp, eos, seed, use_cache=use_cache, return_step_logits=True, return_logprobs=True)
    T = b["input_ids"].shape[1]
    kept = out.shape[1] - T
    assert steps.shape == (kept, tokens.shape[0], cfg.vocab_size) and lp.shape == (tokens.shape[0], kept), (steps.shape, lp.shape, out.shape)
    assert torch.equal(out[:, T:].cpu(), tokens), (out[:, T:].cpu(), tokens)
    close(lp, logprobs, 1e-4, "log-probabilities of the drawn tokens")
    gen = out[:, T:]
    before = torch.cat([torch.zeros_like(gen[:, :1]), (gen == eos).to(torch.int64).cumsum(1)[:, :-1]], dim=1)   # eos tokens before step t
    drawn = steps.permute(1, 0, 2).gather(2, gen[:, :, None])[:, :, 0]   # [R, kept]: the logit of the token drawn at (row, step)
    unfinished = before == 0
    assert bool(unfinished[:, 0].all()) and bool(torch.isfinite(drawn[unfinished]).all()), drawn


@pytest.mark.parametrize("case", ["t64_n1", "t64_n1_eos", "t128_n1"])
def test_sample_graph_replay_equals_eager(case):
    """8: the decode steps replayed from one hipGraph; a new seed and new prompts need no new capture."""
    cfg, sd, batch, n, warp, eos, seed, tokens, logprobs, edge = _e2e(case)
    model = build_model(cfg, sd)
    b = to_dev(batch)
    T = b["input_ids"].shape[1]
    out1 = _sample(model, b, 1, warp, eos, seed, use_graph=True)
    assert torch.equal(out1[:, T:].cpu(), tokens) and torch.equal(out1, _sample(model, b, 1, warp, eos, seed))
    n_graphs = len(model._decode_graphs)
    assert n_graphs == 1
    rolled = {k: torch.roll(v, 1, dims=0) for k, v in b.items()}
    out2, lp2 = _sample(model, rolled, 1, warp, eos, seed + 99, use_graph=True, return_logprobs=True)
    want2, wlp2 = _sample(model, rolled, 1, warp, eos, seed + 99, return_logprobs=True)
    assert torch.equal(out2, want2) and torch.equal(lp2, wlp2)
    assert len(model._decode_graphs) == n_graphs
    assert torch.equal(model.generate(input_ids=b["input_ids"], attention_mask=b["attention_mask"], patch_embeddings=b["patch_embeddings"],
                                      max_new_tokens=3, use_graph=True),
                       model.generate(input_ids=b["input_ids"], attention_mask=b["attention_mask"], patch_embeddings=b["patch_embeddings"],
                                      max_new_tokens=3))   # the greedy graph beside it, under its own key
    assert len(model._decode_graphs) == n_graphs + 1


@pytest.mark.parametrize("case", ["t64_n1", "t64_n3", "t128_n1", "t128_n3_eos"])
def test_sample_bf16_cached_equals_recompute_while_the_margin_is_wide(case):
    """9: bf16: the cached and the recompute paths agree on every row up to the first step whose stored distance of u to the nearest CDF
    edge is below 5e-2 (the beam test's rule for near-ties); beyond that step nothing is asserted."""
    cfg, sd, batch, n, warp, eos, seed, tokens, logprobs, edge = _e2e(case)
    model = build_model(cfg, sd, dtype=torch.bfloat16)
    b = to_dev(batch)
    T = b["input_ids"].shape[1]
    oc = _sample(model, b, n, warp, eos, seed, dtype=torch.bfloat16, use_cache=True)[:, T:].cpu()
    ou = _sample(model, b, n, warp, eos, seed, dtype=torch.bfloat16, use_cache=False)[:, T:].cpu()
    assert oc.shape[0] == ou.shape[0] == tokens.shape[0]
    checked = 0
    for r in range(tokens.shape[0]):
        for t in range(min(oc.shape[1], ou.shape[1])):
            if float(edge[t, r]) < 5e-2:
                break
            assert int(oc[r, t]) == int(ou[r, t]), f"row {r} step {t}: cached {int(oc[r, t])} != recompute {int(ou[r, t])} at margin {float(edge[t, r]):.3e}"
            checked += 1
    print(f"[sample] bf16 {case}: {checked} (row, step) pairs compared")
    # what the stored margins leave to compare (every row's steps before its first narrow one): a regenerated fixture cannot empty the test
    assert checked >= 2 and checked == sum(next((t for t in range(min(oc.shape[1], ou.shape[1])) if float(edge[t, r]) < 5e-2), min(oc.shape[1], ou.shape[1])) for r in range(tokens.shape[0]))


def test_sample_refusals():
    """10."""
    from mafed_amd import _lib, ops
    cfg, sd, batch, n, warp, eos, seed, *_ = _e2e("t64_n1")
    model = build_model(cfg, sd)
    b = to_dev(batch)
    kw = dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], patch_embeddings=b["patch_embeddings"], max_new_tokens=3)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=1.0), dict(min_p=-0.1), dict(top_k=-1),
                dict(num_return_sequences=0), dict(num_return_sequences=9), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            model.sample(**bad, **kw)
    with pytest.raises(NotImplementedError):
        model.generate(do_sample=True, **kw)
    with pytest.raises(NotImplementedError):
        model.sample(use_graph=True, num_return_sequences=2, **kw)
    with pytest.raises(_lib.MafedHipError):   # the kernel's own argument check
        ops.sample_token(torch.zeros(2, 70000, device=DEV), uniforms=torch.full((2,), 0.5, device=DEV))
