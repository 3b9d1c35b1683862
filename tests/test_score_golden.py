"""CPU: the ``model.score`` fixture (tests/golden/score.npz, tools/gen_score_golden.py) against the oracle restatement that wrote it, and
the identity that ties a score to the training loss: -score_mean of a labelled answer is the reference's per-sample masked-mean CE."""
import numpy as np
import pytest
import torch

from oracle import vlpythia_ref as R
from tests.helpers import load_golden
from tests.score_ref import A, C, SCORE_CASES, labelled_batch, ranked_prompts, score_ref, score_setup


def fixture(case):
    g = load_golden("score.npz")
    return {k: torch.from_numpy(g[f"{case}/{k}"]) for k in ("candidate_ids", "candidate_mask", "gold", "token_logprobs", "score_sum", "score_mean")}


@pytest.mark.parametrize("case", SCORE_CASES)
def test_score_ref_reproduces_the_fixture(case):
    cfg, sd, batch = score_setup(case)
    f = fixture(case)
    B = batch["input_ids"].shape[0]
    assert f["candidate_ids"].shape == (B, C, A) and f["candidate_mask"].shape == (B, C, A)
    lengths = f["candidate_mask"].sum(-1)
    assert int(lengths.min()) >= 1 and int(lengths.max()) == A and len(set(lengths.reshape(-1).tolist())) > 1, "ragged lengths 1 .. A"
    tlp, ssum, smean = score_ref(sd, cfg, batch, f["candidate_ids"], f["candidate_mask"])
    # (bit-for-bit on the authoring machine; another thread count may reorder the oracle's sums)
    for got, key in ((tlp, "token_logprobs"), (ssum, "score_sum"), (smean, "score_mean")):
        assert float((got - f[key]).abs().max()) <= 1e-6 * max(1.0, float(f[key].abs().max())), key


@pytest.mark.parametrize("case", SCORE_CASES)
def test_minus_mean_score_of_the_labelled_answer_is_the_training_loss(case):
    cfg, sd, batch = score_setup(case)
    f = fixture(case)
    with torch.no_grad():
        loss = float(R.forward(sd, labelled_batch(batch, f["candidate_ids"], f["candidate_mask"], f["gold"]), cfg).loss)
    ar = torch.arange(f["gold"].shape[0])
    got = float(-f["score_mean"][ar, f["gold"]].mean())
    assert abs(got - loss) <= 1e-5 * max(1.0, abs(loss)), (got, loss)
    assert abs(float(load_golden("score.npz")[f"{case}/loss"]) - loss) <= 1e-5 * max(1.0, abs(loss))


def test_the_fixture_ranks_at_least_half_of_its_prompts():
    ranked = {"score_sum": 0, "score_mean": 0}
    total = 0
    for case in SCORE_CASES:
        f = fixture(case)
        total += f["gold"].shape[0]
        for key in ranked:
            ranked[key] += int(ranked_prompts(f[key]).sum())
    assert min(ranked.values()) * 2 >= total, (ranked, total)
    assert np.isfinite(load_golden("score.npz")["t64/token_logprobs"]).all()
