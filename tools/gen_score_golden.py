"""Authoring tool (CPU): write tests/golden/score.npz, the fixture of ``model.score`` on the decode fixture's models t64, m64, t128 and t256
(tests/score_ref.py: score_setup, score_ref).  Per case: C = 5 candidates of A = 4 tokens per prompt with ragged lengths 1 .. 4
(``candidate_mask`` right-padded); candidate ``gold[b]`` of prompt b is the fixture's own greedy continuation (the oracle's
``generate_greedy`` without an eos; where decode.npz holds the case, its tokens), the rest are random ids; token log-probabilities and both
scores from the oracle on the expanded sequences.  The candidates' seed is searched until the ranking condition of the tests holds --
under each normalisation, at least half of all prompts have a top-2 score gap above 1e-2 x max|score| -- and that is asserted before
anything is written.

    python tools/gen_score_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vlpythia_ref as R  # noqa: E402
from tests.helpers import DECODE_CASES, GOLDEN, decode_setup  # noqa: E402
from tests.score_ref import A, C, SCORE_CASES, labelled_batch, ranked_prompts, score_ref, score_setup  # noqa: E402


def candidates(cfg, batch, greedy, seed):
    B = greedy.shape[0]
    rs = np.random.RandomState(seed)
    cand = torch.from_numpy(rs.randint(1, cfg.vocab_size, size=(B, C, A)).astype(np.int64))
    gold = torch.arange(B) % C
    cand[torch.arange(B), gold] = greedy
    length = 1 + (torch.arange(B)[:, None] + torch.arange(C)[None, :]) % A          # ragged: 1 .. A
    mask = (torch.arange(A)[None, None, :] < length[:, :, None]).to(torch.int64)
    return cand, mask, gold


def main():
    torch.manual_seed(0)
    setups = {}
    for case in SCORE_CASES:
        cfg, sd, batch = score_setup(case)
        T = batch["input_ids"].shape[1]
        greedy = R.generate_greedy(sd, batch, cfg, max_new_tokens=A, eos_token_id=None)[0][:, T:]
        if case in DECODE_CASES:
            _, _, _, eos, max_new, tokens, *_ = decode_setup(case)
            if eos is None:
                n = min(A, tokens.shape[1] - T)
                assert torch.equal(tokens[:, T:T + n], greedy[:, :n]), f"{case}: greedy continuation differs from decode.npz"
        setups[case] = (cfg, sd, batch, greedy)
    for seed in range(100):
        out, ranked, total = {"seed": np.int64(seed)}, {"sum": 0, "mean": 0}, 0
        for case, (cfg, sd, batch, greedy) in setups.items():
            cand, mask, gold = candidates(cfg, batch, greedy, 1000 * seed + len(case) + cfg.vocab_size)
            tlp, ssum, smean = score_ref(sd, cfg, batch, cand, mask)
            total += cand.shape[0]
            ranked["sum"] += int(ranked_prompts(ssum).sum())
            ranked["mean"] += int(ranked_prompts(smean).sum())
            loss = float(R.forward(sd, labelled_batch(batch, cand, mask, gold), cfg).loss)
            ar = torch.arange(cand.shape[0])
            assert abs(loss - float(-smean[ar, gold].mean())) <= 1e-5 * max(1.0, abs(loss)), (case, loss)
            for k, v in (("candidate_ids", cand), ("candidate_mask", mask), ("gold", gold), ("token_logprobs", tlp), ("score_sum", ssum),
                         ("score_mean", smean)):
                out[f"{case}/{k}"] = v.numpy()
            out[f"{case}/loss"] = np.float32(loss)
        print(f"seed {seed}: ranked prompts {ranked} of {total}")
        if min(ranked.values()) * 2 >= total:
            break
    assert min(ranked.values()) * 2 >= total, "no seed meets the ranking condition"
    path = os.path.join(GOLDEN, "score.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
