"""Golden beam-search fixture (tests/golden/beam.npz): ``generate(num_beams=k)`` as transformers' own
``GenerationMixin._beam_search`` runs it, on a ``GPTNeoXForCausalLM`` that holds the oracle's weights.

The installed transformers no longer mixes ``generate`` into the reference class, so the search runs on the plain GPT-NeoX
with the VLPythia input built around it: every forward receives ``inputs_embeds = [projector(patch) | embed_in(ids)]``, the
mask ``[ones(P) | attention_mask | ones(generated)]``, ``arange`` positions (HF's own
``prepare_inputs_for_generation`` would derive them from the mask) and ``use_cache=False``.  Every forward's logits are
asserted against ``oracle.vlpythia_ref.forward`` on the same sequences.  A plain restatement of the search
(``beam_search_restated``) runs beside it on the oracle's logits and must agree; it also yields the smallest score gap
between adjacent ranks 0 .. 2k of every step's candidate list, per sample, so tests can tell where a tie could flip a
choice under a different rounding.

    python tools/gen_beam_golden.py          # rewrites tests/golden/beam.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import vlpythia_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "beam.npz")
SEED = 89

TINY = {  # (mirrors tests/helpers.py::TINY)
    "t64": dict(h=128, H=2, L=3, V=512, P=8, T=6, B=3, Dv=32),
    "t128": dict(h=256, H=2, L=2, V=256, P=8, T=6, B=2, Dv=32),
    "m64": dict(h=128, H=2, L=4, V=600, P=40, T=24, B=3, Dv=48),
}

# case -> (tiny config, num_beams, left padding, eos ("pick": a token the search emits, so hypotheses finish early),
#          length_penalty, early_stopping, num_return_sequences, max_new_tokens)
CASES = {
    "t64_k2": ("t64", 2, True, None, 1.0, False, 1, 6),
    "t64_k3_eos": ("t64", 3, True, "pick", 1.0, False, 2, 7),
    "t64_k3_eos_lp06": ("t64", 3, True, "pick", 0.6, True, 1, 7),
    "t64_k5_eos_lp2_never": ("t64", 5, False, "pick", 2.0, "never", 3, 6),
    "t64_k3_eos_early": ("t64", 3, False, "pick", 1.0, True, 3, 8),
    "m64_k3": ("m64", 3, True, "pick", 1.0, False, 1, 5),
    "t128_k2_nopad": ("t128", 2, False, None, 2.0, "never", 2, 5),
    "t128_k5_eos": ("t128", 5, True, "pick", 0.6, False, 2, 6),
}


def tiny_cfg(name):
    t = TINY[name]
    return R.RefConfig(vocab_size=t["V"], hidden_size=t["h"], num_hidden_layers=t["L"], num_attention_heads=t["H"],
                       intermediate_size=4 * t["h"], vision_hidden_size=t["Dv"], num_vision_tokens=t["P"])


def case_inputs(case, eos_id=None):
    """(cfg, weights, batch, params) of one case; params = dict(k, eos, lp, early, nrs, max_new).  ``eos_id``: the fixture's recorded
    eos id of a "pick" case (a consumer of the committed fixture passes it instead of re-deriving it through the oracle)."""
    name, k, pad, eos, lp, early, nrs, max_new = CASES[case]
    cfg, t = tiny_cfg(name), TINY[name]
    sd = R.init_weights(cfg, seed=SEED)
    batch = R.make_batch(cfg, t["B"], t["T"], seed=SEED + 1, pad=pad)
    if eos == "pick" and eos_id is not None:
        eos = int(eos_id)
    elif eos == "pick":
        # the token sample 0's best beam emits at its third step: with random weights no fixed id is ever likely
        seqs, _, _ = beam_search_restated(sd, batch, cfg, k, None, None, 1.0, False, 1, max_new)
        eos = int(seqs[0, t["T"] + 2])
    return cfg, sd, batch, dict(k=k, eos=eos, lp=lp, early=early, nrs=nrs, max_new=max_new)


def oracle_logits(sd, cfg, feats, ids, am):
    with torch.no_grad():
        return R.forward(sd, {"input_ids": ids, "attention_mask": am, "patch_embeddings": feats}, cfg).logits[:, -1, :].float()


def beam_search_restated(sd, batch, cfg, k, eos, pad, lp, early, nrs, max_new):
    """transformers 5.x ``_beam_search`` (one eos id, no logits processors) written out per sample, on the oracle's logits.
    Returns (sequences [B * nrs, T + n], normalised scores [B * nrs], smallest adjacent gap of ranks 0 .. 2k per sample [B])."""
    ids0, am0, feats0 = batch["input_ids"], batch["attention_mask"], batch["patch_embeddings"]
    B, T = ids0.shape
    V = cfg.vocab_size
    fill = (pad or eos) if eos is not None else -1
    run_tok = [[[] for _ in range(k)] for _ in range(B)]
    run_score = torch.full((B, k), -1e9)
    run_score[:, 0] = 0.0
    fin = [[(-1e9, None) for _ in range(k)] for _ in range(B)]   # (normalised score, tokens or None)
    unsat = [True] * B
    gaps = torch.full((B,), float("inf"))
    for n in range(max_new):
        ids = torch.cat([ids0.repeat_interleave(k, 0), torch.tensor([run_tok[b][r] for b in range(B) for r in range(k)], dtype=torch.int64).view(B * k, n)], 1)
        am = torch.cat([am0.repeat_interleave(k, 0), torch.ones(B * k, n, dtype=torch.int64)], 1)
        lg = oracle_logits(sd, cfg, feats0.repeat_interleave(k, 0), ids, am)
        acc = (F.log_softmax(lg, -1).view(B, k, V) + run_score[:, :, None]).view(B, k * V)
        last = n == max_new - 1
        for b in range(B):
            vals, idx = torch.topk(acc[b], 2 * k + 1)
            gaps[b] = min(float(gaps[b]), float((vals[:-1] - vals[1:]).min()))
            vals, idx = vals[:2 * k], idx[:2 * k]
            par, tok = (idx // V).tolist(), (idx % V).tolist()
            hit = [last or (eos is not None and t_ == eos) for t_ in tok]
            full = all(s is not None for _, s in fin[b]) and early is True
            if unsat[b] and not full:
                new = [(float(vals[i]) / float((n + 1) ** lp), run_tok[b][par[i]] + [tok[i]]) for i in range(k) if hit[i]]
                merged = fin[b] + new
                order = sorted(range(len(merged)), key=lambda i: -merged[i][0])   # stable: earlier entries first on ties
                fin[b] = [merged[i] for i in order[:k]]
            keep = [i for i in range(2 * k) if not hit[i]][:k] if not last else list(range(k))
            run_tok[b] = [run_tok[b][par[i]] + [tok[i]] for i in keep]
            run_score[b] = torch.tensor([float(vals[i]) for i in keep])
            if early == "never" and lp > 0.0:
                best_len = max_new
            else:
                best_len = n + 1
            best = float(run_score[b, 0]) / float(best_len ** lp)
            all_fin = all(s is not None for _, s in fin[b])
            worst = min(sc for sc, _ in fin[b]) if all_fin else -1e9
            unsat[b] = unsat[b] and best > worst
    rows = [fin[b][i] for b in range(B) for i in range(nrs)]
    n_out = max(len(s) for _, s in rows)
    seqs = torch.full((B * nrs, T + n_out), fill, dtype=torch.int64)
    seqs[:, :T] = ids0.repeat_interleave(nrs, 0)
    for i, (_, s) in enumerate(rows):
        seqs[i, T:T + len(s)] = torch.tensor(s, dtype=torch.int64)
    return seqs, torch.tensor([sc for sc, _ in rows], dtype=torch.float32), gaps


def hf_beam_search(sd, batch, cfg, k, eos, pad, lp, early, nrs, max_new):
    """transformers' own search on GPTNeoXForCausalLM (weights from ``sd``); returns (sequences, sequences_scores)."""
    from transformers import GenerationConfig, GPTNeoXConfig, GPTNeoXForCausalLM

    hc = GPTNeoXConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                       num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                       rotary_pct=cfg.rotary_pct, rotary_emb_base=cfg.rotary_emb_base, max_position_embeddings=2048,
                       layer_norm_eps=cfg.layer_norm_eps, tie_word_embeddings=False, hidden_dropout=0.0, attention_dropout=0.0,
                       use_parallel_residual=True, attention_bias=True, hidden_act="gelu", bos_token_id=None, eos_token_id=None,
                       pad_token_id=None)
    hc._attn_implementation = "eager"
    P = cfg.num_vision_tokens
    feats0 = batch["patch_embeddings"]

    class VLNeoX(GPTNeoXForCausalLM):
        """input_ids = [prompt | generated]: the image prefix is spliced in front of them on every call."""

        def forward(self, input_ids=None, attention_mask=None, position_ids=None, use_cache=None, **kw):
            rows, n = input_ids.shape
            feats = feats0.repeat_interleave(rows // feats0.shape[0], 0)
            img = F.linear(F.gelu(F.linear(feats, sd["vision_embed_tokens.0.weight"], sd["vision_embed_tokens.0.bias"])),
                           sd["vision_embed_tokens.2.weight"], sd["vision_embed_tokens.2.bias"])
            emb = torch.cat([img, self.gpt_neox.embed_in(input_ids)], 1)
            am = torch.cat([torch.ones(rows, P, dtype=attention_mask.dtype), attention_mask], 1)
            pos = torch.arange(P + n)[None, :].expand(rows, -1)
            keep = {key: v for key, v in kw.items() if key in ("return_dict", "output_attentions", "output_hidden_states")}
            out = super().forward(inputs_embeds=emb, attention_mask=am, position_ids=pos, use_cache=False, **keep)
            want = oracle_logits(sd, cfg, feats, input_ids, attention_mask)
            got = out.logits[:, -1, :].float()
            assert float((got - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max())), "GPT-NeoX forward != oracle forward"
            return out

    model = VLNeoX(hc)
    # (the installed class names the LM head ``lm_head``; the reference checkpoint ``embed_out``)
    neox = {("lm_head.weight" if k_ == "embed_out.weight" else k_): v for k_, v in sd.items() if not k_.startswith("vision_embed_tokens")}
    missing, unexpected = model.load_state_dict(neox, strict=False)
    assert not unexpected, unexpected
    assert all("rotary" in m for m in missing), missing
    model.eval()
    gc = GenerationConfig(num_beams=k, do_sample=False, max_new_tokens=max_new, length_penalty=lp, early_stopping=early,
                          num_return_sequences=nrs, eos_token_id=eos, pad_token_id=pad, bos_token_id=None, use_cache=False,
                          return_dict_in_generate=True, output_scores=True)
    with torch.no_grad():
        out = model.generate(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], generation_config=gc)
    return out.sequences, out.sequences_scores.float()


def run_case(case):
    """(params, sequences, scores, gaps) of one case; transformers and the restatement must agree."""
    cfg, sd, batch, p = case_inputs(case)
    pad = p["eos"]
    seqs, scores = hf_beam_search(sd, batch, cfg, p["k"], p["eos"], pad, p["lp"], p["early"], p["nrs"], p["max_new"])
    s2, sc2, gaps = beam_search_restated(sd, batch, cfg, p["k"], p["eos"], pad, p["lp"], p["early"], p["nrs"], p["max_new"])
    assert torch.equal(seqs, s2), (case, seqs, s2)
    assert float((scores - sc2).abs().max()) < 1e-5, (case, scores, sc2)
    return p, seqs, scores, gaps


EARLY_CODE = {False: 0, True: 1, "never": 2}


def main():
    torch.manual_seed(0)
    out = {"seed": np.int64(SEED)}
    for case in CASES:
        p, seqs, scores, gaps = run_case(case)
        out[f"{case}/sequences"] = seqs.numpy()
        out[f"{case}/scores"] = scores.numpy()
        out[f"{case}/gap"] = gaps.numpy()
        out[f"{case}/eos"] = np.int64(-1 if p["eos"] is None else p["eos"])
        T = TINY[CASES[case][0]]["T"]
        print(f"beam fixture {case}: k={p['k']} eos={p['eos']} lp={p['lp']} early={p['early']} nrs={p['nrs']} -> {tuple(seqs.shape)}, "
              f"generated {seqs.shape[1] - T}, min gap {float(gaps.min()):.3e}, scores {scores.tolist()}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
