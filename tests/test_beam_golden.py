"""CPU: the beam-search fixture (tests/golden/beam.npz) is what transformers' own GenerationMixin._beam_search computes on a
GPT-NeoX holding the oracle's weights (tools/gen_beam_golden.py), and the restatement beside it agrees."""
import numpy as np
import pytest

from tests.helpers import load_golden

pytest.importorskip("transformers")

from tools import gen_beam_golden as G  # noqa: E402


@pytest.mark.parametrize("case", list(G.CASES))
def test_beam_fixture_regenerates_from_transformers_and_the_oracle(case):
    g = load_golden("beam.npz")
    assert int(g["seed"]) == G.SEED
    p, seqs, scores, gaps = G.run_case(case)   # (asserts transformers == restatement and every forward == the oracle's)
    assert int(g[f"{case}/eos"]) == (-1 if p["eos"] is None else p["eos"])
    assert np.array_equal(seqs.numpy(), g[f"{case}/sequences"]), case
    assert np.abs(scores.numpy() - g[f"{case}/scores"]).max() < 1e-5
    assert np.allclose(gaps.numpy(), g[f"{case}/gap"], rtol=1e-3, atol=1e-6)


def test_beam_fixture_covers_the_issue_cases():
    ks = {c[1] for c in G.CASES.values()}
    assert {2, 3, 5} <= ks
    assert {True, False} <= {c[2] for c in G.CASES.values()}                 # left padding on and off
    assert any(c[3] == "pick" for c in G.CASES.values())                      # hypotheses that finish early
    assert {1.0, 0.6, 2.0} <= {c[4] for c in G.CASES.values()}
    assert [False, True, "never"] == sorted({c[5] for c in G.CASES.values()}, key=lambda e: {False: 0, True: 1, "never": 2}[e])
    assert any(c[6] > 1 for c in G.CASES.values())
    g = load_golden("beam.npz")
    for case in G.CASES:
        assert g[f"{case}/sequences"].shape[0] == G.TINY[G.CASES[case][0]]["B"] * G.CASES[case][6]
    # early finishers: some returned hypothesis is shorter than the longest one (its tail is the pad id)
    assert any(int(g[f"{c}/eos"]) >= 0 and (g[f"{c}/sequences"][:, -1] == int(g[f"{c}/eos"])).any() for c in G.CASES)
