"""CPU: the sampling fixture (tests/golden/sample.npz, tools/gen_sample_golden.py) and the numpy restatement it was made with
(tests/sample_ref.py): Philox4x32-10 known answers, the kept masks regenerated from transformers' warpers, the stored margins."""
import numpy as np
import pytest

from tests import sample_ref as S
from tests.helpers import load_golden

KERNEL_CASES = [(r, V, s) for r in S.RECIPES for V in S.VOCABS for s in range(len(S.PARAM_SETS))]


def test_philox4x32_10_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(x) for x in S.philox4x32_10(ctr, key))
        assert got == want, (ctr, key, [hex(x) for x in got])


def test_uniforms_are_fp32_values_keyed_by_row_and_step():
    u = S.uniforms(0x123456789abcdef0, 7, 3)
    assert u.shape == (7,) and np.all(u > 0) and np.all(u <= 1) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert np.array_equal(S.uniforms(0x123456789abcdef0, 3, 3), u[:3])
    assert not np.array_equal(S.uniforms(0x123456789abcdef0, 7, 4), u) and not np.array_equal(S.uniforms(0x023456789abcdef0, 7, 3), u)


@pytest.mark.parametrize("recipe,V,s", KERNEL_CASES)
def test_fixture_masks_regenerate_from_the_warpers(recipe, V, s):
    g = load_golden("sample.npz")
    pre = f"k/{recipe}/{V}/{s}/"
    T, k, p, mp = S.PARAM_SETS[s]
    logits = S.case_logits(recipe, V, int(g[pre + "seed"]))
    chk = float(logits.double().abs().sum())
    assert abs(chk - float(g[pre + "checksum"])) <= 1e-9 * chk, "the logit recipe drifted"
    stored = S.unpack_mask(g[pre + "mask"], V)
    mask, margin = S.kept_by_value(logits, T, k, p, mp)
    assert np.array_equal(mask, stored)
    # no threshold decision within the case's margin of its cut (the generator's condition)
    assert float(margin.min()) >= S.case_margin(recipe, V, s) and np.array_equal(margin, g[pre + "margin"])
    # transformers' own warpers give the same mask, up to the ids of an exact tie on the top-p cut (kept whole here)
    hf = S.hf_mask(logits, T, k, p, mp).numpy()
    z = logits.double().numpy() / T
    assert int((hf != stored).sum()) == int(g[pre + "hf_differs"])
    for r in range(S.ROWS):
        diff = hf[r] != stored[r]
        assert not (hf[r] & ~stored[r]).any()
        assert np.all(z[r][diff] == z[r][hf[r]].min())
    # the stored tokens are the fp64 inverse CDF of the stored uniforms
    u = g[pre + "uniforms"]
    for r in range(S.ROWS):
        assert S.draw(S.cdf(logits[r].numpy(), T, stored[r])[1], stored[r], float(u[r])) == int(g[pre + "tokens"][r])


def test_end_to_end_cases_keep_their_draws_away_from_the_cdf_edges():
    g = load_golden("sample.npz")
    cases = sorted({key.split("/")[1] for key in g.files if key.startswith("e/")})
    assert len(cases) == 12
    for case in cases:
        edge, u, seed = g[f"e/{case}/edge"], g[f"e/{case}/uniforms"], int(g[f"e/{case}/seed"])
        assert float(edge.min()) >= 1e-3 and float(g[f"e/{case}/margin"]) >= 2e-3
        for t in range(u.shape[0]):
            assert np.array_equal(S.uniforms(seed, u.shape[1], t), u[t])
