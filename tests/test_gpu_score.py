"""GPU: ``model.score`` (candidate log-likelihoods over one shared prompt prefill, DESIGN.md section 4c'''') against the oracle fixture
tests/golden/score.npz, against the training loss, and shared against expanded; ``ops.token_logprob`` against float64 log_softmax."""
import inspect

import pytest
import torch

from tests.helpers import load_golden
from tests.score_ref import A, C, SCORE_CASES, labelled_batch, ranked_prompts, score_setup
from tests.test_gpu_model import DEV, build_model, close, to_dev
from tests.test_gpu_shared_image import CROSS_IMAGE, CROSS_TEXT

pytestmark = pytest.mark.gpu

# Error of the EXPANDED bf16 path (use_cache=False: the engine forward and the existing attention kernels) against the fp32 fixture, token
# log-probabilities under `close`; the shared path is held to max(3e-2, 2 x this) against the expanded one.  NOT YET MEASURED on an MI355X
# (the test prints it): 0 leaves the bound at 3e-2, the tighter of the two.
E_EXPANDED_BF16 = {"t64": 0.0, "m64": 0.0, "t128": 0.0}


def fixture(case):
    g = load_golden("score.npz")
    return {k: torch.from_numpy(g[f"{case}/{k}"]) for k in ("candidate_ids", "candidate_mask", "gold", "token_logprobs", "score_sum", "score_mean")}


def score_kwargs(batch, f):
    b = to_dev(batch)
    return dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], patch_embeddings=b["patch_embeddings"],
                candidate_ids=f["candidate_ids"].to(DEV), candidate_mask=f["candidate_mask"].to(DEV))


# ---- ops.token_logprob ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 8, 3])          # row stride V, V + 8 (vector loads) and V + 3 (rows off the 4-element grid)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [50304, 1000])
def test_token_logprob_vs_float64_log_softmax(V, dt, pad):
    from mafed_amd import ops
    g = torch.Generator().manual_seed(V + pad)
    N, R = 6, 10
    store = (torch.randn(N, V + pad, generator=g) * 4.0).to(dt).to(DEV)
    logits = store[:, :V]
    rows = torch.tensor([5, 0, 0, 3, 1, 1, 1, 4, 2, 5], dtype=torch.int32, device=DEV)
    target = torch.randint(0, V, (R,), generator=g)
    target[2], target[7] = -1, -100                  # masked positions
    target[4], target[5] = 0, V - 1
    ref = torch.log_softmax(logits.cpu().double(), dim=-1)   # on the very values the kernel reads (bf16 included)
    scale = float(logits.abs().max())
    keep = target >= 0
    want = torch.where(keep, ref[rows.cpu().long(), target.clamp(min=0)], torch.zeros(R, dtype=torch.float64))
    got = ops.token_logprob(logits, target.to(DEV), rows)
    err = float((got.cpu().double() - want).abs().max())
    print(f"[token_logprob] V {V} {dt} pad {pad}: max err {err:.3e} = {err / scale:.3e} x max|logit|")
    assert got.dtype == torch.float32 and err <= 1e-5 * scale
    assert bool((got[~keep.to(DEV)] == 0).all())
    assert torch.equal(got, ops.token_logprob(logits, target.to(DEV), rows)), "a second call gives the same bits"
    # no map: output r reads row r; a row's result does not depend on R or on the other rows
    t6 = target[:N].clamp(min=0).to(DEV)
    got6 = ops.token_logprob(logits, t6)
    want6 = ref[torch.arange(N), t6.cpu()]
    assert float((got6.cpu().double() - want6).abs().max()) <= 1e-5 * scale
    assert torch.equal(ops.token_logprob(logits[:2], t6[:2]), got6[:2])


def test_score_reduce_sums_means_and_empty_candidates():
    from mafed_amd import ops
    tlp = -torch.rand(3, 5, 4, device=DEV)
    mask = (torch.arange(4, device=DEV)[None, None, :] < torch.tensor([[0, 1, 2, 3, 4]] * 3, device=DEV)[:, :, None]).to(torch.int64)
    s, m = ops.score_reduce(tlp, mask, False), ops.score_reduce(tlp, mask, True)
    assert bool(torch.isinf(s[:, 0]).all()) and bool((s[:, 0] < 0).all()) and bool(torch.isinf(m[:, 0]).all())
    want = (tlp * mask).sum(-1)
    close(s[:, 1:], want[:, 1:], 1e-6, "sum")
    close(m[:, 1:], (want / mask.sum(-1).clamp(min=1))[:, 1:], 1e-6, "mean")
    close(ops.score_reduce(tlp, None, False), tlp.sum(-1), 1e-6, "no mask")


# ---- model.score ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_cache", [True, False])
def test_score_fp32_matches_the_fixture(use_cache):
    """Token log-probabilities and both scores of all four cases at the project's parity bar; the same best candidate for every prompt
    whose fixture top-2 gap exceeds 1e-2 x max|score| -- at least half of all prompts, under each normalisation."""
    compared = {"sum": 0, "mean": 0}
    total = 0
    for case in SCORE_CASES:
        cfg, sd, batch = score_setup(case)
        f = fixture(case)
        model = build_model(cfg, sd)
        kw = score_kwargs(batch, f)
        ssum, tlp = model.score(use_cache=use_cache, return_token_logprobs=True, **kw)
        smean = model.score(use_cache=use_cache, normalize="mean", **kw)
        assert ssum.shape == (tlp.shape[0], C) and tlp.shape[1:] == (C, A) and ssum.dtype == tlp.dtype == torch.float32
        for got, key in ((tlp, "token_logprobs"), (ssum, "score_sum"), (smean, "score_mean")):
            err = float((got.cpu() - f[key]).abs().max())
            print(f"[score] {case} use_cache={use_cache} {key}: max err {err:.3e}")
            close(got, f[key], 1e-3, f"{case} {key}")
        assert bool((tlp.cpu()[f["candidate_mask"] == 0] == 0).all())
        total += ssum.shape[0]
        for norm, got, key in (("sum", ssum, "score_sum"), ("mean", smean, "score_mean")):
            ranked = ranked_prompts(f[key])
            assert torch.equal(got.argmax(-1).cpu()[ranked], f[key].argmax(-1)[ranked]), (case, norm)
            compared[norm] += int(ranked.sum())
    print(f"[score] best candidate compared for {compared} of {total} prompts")
    assert min(compared.values()) * 2 >= total


@pytest.mark.parametrize("case", SCORE_CASES)
def test_minus_mean_score_of_the_labelled_answer_is_the_model_loss(case):
    cfg, sd, batch = score_setup(case)
    f = fixture(case)
    model = build_model(cfg, sd)
    smean = model.score(normalize="mean", **score_kwargs(batch, f))
    with torch.no_grad():
        loss = float(model(**to_dev(labelled_batch(batch, f["candidate_ids"], f["candidate_mask"], f["gold"]))).loss)
    got = float(-smean[torch.arange(smean.shape[0], device=DEV), f["gold"].to(DEV)].mean())
    print(f"[score] {case}: batch mean of -score_mean {got:.6f}, model loss {loss:.6f}")
    assert abs(got - loss) <= 1e-3 * max(1.0, abs(loss))


def test_score_shared_image_equals_expanded_features():
    """Prompts and images paired across the fixture's rows (tests/test_gpu_shared_image.py): ``image_index`` against the same call on
    ``patch_embeddings[image_index]``, on both paths."""
    cfg, sd, batch = score_setup("t64")
    f = fixture("t64")
    model = build_model(cfg, sd)
    b = to_dev(batch)
    t, im = torch.tensor(CROSS_TEXT, device=DEV), torch.tensor(CROSS_IMAGE, device=DEV)
    kw = dict(input_ids=b["input_ids"][t].contiguous(), attention_mask=b["attention_mask"][t].contiguous(),
              candidate_ids=f["candidate_ids"].to(DEV)[t].contiguous(), candidate_mask=f["candidate_mask"].to(DEV)[t].contiguous(),
              return_token_logprobs=True)
    want_s, want_t = model.score(patch_embeddings=b["patch_embeddings"][im].contiguous(), **kw)
    model.prefill_trace = []
    got_s, got_t = model.score(patch_embeddings=b["patch_embeddings"], image_index=im, **kw)
    close(got_t, want_t, 1e-3, "token log-probabilities, shared image")
    close(got_s, want_s, 1e-3, "scores, shared image")
    P, T = cfg.num_vision_tokens, b["input_ids"].shape[1]
    assert model.prefill_trace == [{"prefix_rows": 3 * P + 6 * T, "candidate_rows": 6 * C * A}]
    lit_s, lit_t = model.score(patch_embeddings=b["patch_embeddings"], image_index=im.cpu(), use_cache=False, **kw)
    close(lit_t, want_t, 1e-3, "token log-probabilities, literal path on feats[image_index]")
    close(lit_s, want_s, 1e-3, "scores, literal path on feats[image_index]")


def test_score_moves_the_prompt_through_the_stack_once():
    """B = 3, C = 5: 3 * S0 prefix rows and 3 * 5 * A_run candidate rows, not 15 * (S0 + A); a padded run length gives the same scores."""
    cfg, sd, batch = score_setup("t64")
    f = fixture("t64")
    model = build_model(cfg, sd)
    kw = score_kwargs(batch, f)
    S0 = cfg.num_vision_tokens + batch["input_ids"].shape[1]
    model.prefill_trace = []
    plain_s, plain_t = model.score(return_token_logprobs=True, **kw)
    assert model.padded_candidate_len(3 * C, A) == A
    assert model.prefill_trace == [{"prefix_rows": 3 * S0, "candidate_rows": 3 * C * A}]
    model.score(use_cache=False, **kw)
    assert len(model.prefill_trace) == 1, "the literal path has no shared prefill to report"
    model.text_bucket = 8          # candidates run at A_run = 8: the padded rows come last in their candidate and nobody else sees them
    assert model.padded_candidate_len(3 * C, A) == 8
    pad_s, pad_t = model.score(return_token_logprobs=True, **kw)
    assert model.prefill_trace[-1] == {"prefix_rows": 3 * S0, "candidate_rows": 3 * C * 8}
    close(pad_t, plain_t, 1e-5, "token log-probabilities at the padded run length")   # (fp32 rounding: the row count may change a GEMM's tiles)
    close(pad_s, plain_s, 1e-5, "scores at the padded run length")
    # one token per candidate: scored from the prompt's last position alone, no candidate row enters the stack
    one = dict(kw, candidate_ids=kw["candidate_ids"][:, :, :1].contiguous(), candidate_mask=None)
    s1, t1 = model.score(return_token_logprobs=True, **one)
    assert model.prefill_trace[-1] == {"prefix_rows": 3 * S0, "candidate_rows": 0}
    close(t1[:, :, 0], plain_t[:, :, 0], 1e-5, "first-token log-probabilities")
    close(s1, t1[:, :, 0], 0.0, "one-token scores")


@pytest.mark.parametrize("case", ["t64", "m64", "t128"])
def test_score_bf16_shared_tracks_expanded(case):
    """bf16 (MFMA) mode: the shared path's token log-probabilities against the expanded path's, within max(3e-2, 2 e) -- 3e-2 is the bound
    of test_gpu_shared_image for shared-vs-unshared bf16 logits, e the expanded path's own error against the fp32 fixture, and a
    log-probability is a difference of two such quantities."""
    cfg, sd, batch = score_setup(case)
    f = fixture(case)
    model = build_model(cfg, sd, dtype=torch.bfloat16)
    kw = score_kwargs(batch, f)
    kw["patch_embeddings"] = kw["patch_embeddings"].to(torch.bfloat16)
    exp_s, exp_t = model.score(use_cache=False, return_token_logprobs=True, **kw)
    sh_s, sh_t = model.score(use_cache=True, return_token_logprobs=True, **kw)
    scale = max(1.0, float(f["token_logprobs"].abs().max()))
    e_now = float((exp_t.cpu() - f["token_logprobs"]).abs().max()) / scale
    d = float((sh_t - exp_t).abs().max()) / max(1.0, float(exp_t.abs().max()))
    bound = max(3e-2, 2 * E_EXPANDED_BF16[case])
    print(f"[score bf16] {case}: expanded vs fp32 fixture {e_now:.3e}, shared vs expanded {d:.3e} (bound {bound:.1e})")
    assert bool(torch.isfinite(sh_t).all())
    close(sh_t, exp_t, bound, f"{case}: shared vs expanded token log-probabilities")


def test_score_edge_cases_and_errors():
    cfg, sd, batch = score_setup("t64")
    f = fixture("t64")
    model = build_model(cfg, sd)
    kw = score_kwargs(batch, f)
    assert "candidate_ids" in inspect.signature(model.score).parameters
    cand, mask = kw["candidate_ids"], kw["candidate_mask"]
    B = cand.shape[0]
    for use_cache in (True, False):
        # a candidate without a token loses every ranking
        m0 = mask.clone()
        m0[:, 2] = 0
        for norm in ("sum", "mean"):
            s = model.score(**dict(kw, candidate_mask=m0), normalize=norm, use_cache=use_cache)
            assert bool(torch.isinf(s[:, 2]).all()) and bool((s[:, 2] < 0).all()) and bool(torch.isfinite(s[:, [0, 1, 3, 4]]).all())
            assert bool((s.argmax(-1) != 2).all())
        # no mask = a mask of ones; ids under a zero of the mask are never looked up
        s_none = model.score(**dict(kw, candidate_mask=None), use_cache=use_cache)
        s_ones = model.score(**dict(kw, candidate_mask=torch.ones_like(mask)), use_cache=use_cache)
        assert torch.equal(s_none, s_ones)
        wild = torch.where(mask != 0, cand, torch.full_like(cand, -100))
        assert torch.equal(model.score(**dict(kw, candidate_ids=wild), use_cache=use_cache), model.score(use_cache=use_cache, **kw))
    bad_ids = [cand.to(torch.int32), cand[:, :, 0], cand[:B - 1], cand[:, :, :0], cand[:, :0], cand.tolist(), None,
               cand.clone().fill_(cfg.vocab_size)]
    for bad in bad_ids:
        with pytest.raises(ValueError):
            model.score(**dict(kw, candidate_ids=bad))
    left = mask.clone()
    left[0, 0] = torch.tensor([0, 1, 1, 1], device=DEV)
    twos = mask.clone()
    twos[0, 0, 0] = 2
    for bad in (mask[:, :, :3], mask.to(torch.int32), mask.bool(), left, twos, mask.tolist()):
        with pytest.raises(ValueError):
            model.score(**dict(kw, candidate_mask=bad))
    with pytest.raises(ValueError):
        model.score(normalize="max", **kw)
    with pytest.raises(ValueError):
        model.score(**dict(kw, input_ids=None))
    for bad in (torch.zeros(B + 1, dtype=torch.int64, device=DEV), torch.tensor([0] * (B - 1) + [B], device=DEV), torch.zeros(B, dtype=torch.int32)):
        with pytest.raises(ValueError):
            model.score(image_index=bad, **kw)
    with pytest.raises(ValueError):   # N != B and no index to pair them
        model.score(**dict(kw, patch_embeddings=kw["patch_embeddings"][:B - 1]))
