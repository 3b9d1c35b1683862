"""GPU: ``generate`` / ``sample`` with ``image_index`` -- several prompts about one image, the image rows prefilled once per image
(DESIGN.md section 4c''') -- against the golden decode fixtures and against the same calls on expanded features."""
import inspect

import pytest
import torch

from tests.helpers import DECODE_CASES, decode_setup
from tests.test_gpu_model import DEV, build_model, close, to_dev

pytestmark = pytest.mark.gpu

# cross pairings of the three fixture prompts (twice each) with the three fixture images.  The first serves image 0 to four prompts; the
# second leaves image 1 unused.  On the CPU oracle (generate_greedy on the crossed batch) the smallest top-2 gap exceeds 1e-2 x max|logit| at
# 7 of the 16 steps of t64 + m64 under the first pairing and at 12 of 16 under the second: 19 of 32 together; the smallest gap of any
# step is 1.4e-4 x max|logit|, two orders above fp32 rounding, so the runs stay on one path throughout.
CROSS_TEXT = [0, 1, 2, 0, 1, 2]
CROSS_IMAGE = [0, 0, 0, 1, 2, 1]
CROSS_IMAGE_2 = [0, 0, 0, 0, 0, 2]


def _idx(values):
    return torch.tensor(values, dtype=torch.int64, device=DEV)


def _doubled(b, feats_dtype=None):
    """The fixture's prompts twice over the fixture's features once: (generate kwargs with image_index, the same on expanded features)."""
    B = b["input_ids"].shape[0]
    feats = b["patch_embeddings"] if feats_dtype is None else b["patch_embeddings"].to(feats_dtype)
    ids, am = b["input_ids"].repeat(2, 1), b["attention_mask"].repeat(2, 1)
    shared = dict(input_ids=ids, attention_mask=am, patch_embeddings=feats, image_index=_idx(list(range(B)) * 2))
    plain = dict(input_ids=ids, attention_mask=am, patch_embeddings=feats.repeat(2, 1, 1))
    return shared, plain


def _crossed(b, images=CROSS_IMAGE):
    t, im = _idx(CROSS_TEXT), _idx(images)
    ids, am = b["input_ids"][t].contiguous(), b["attention_mask"][t].contiguous()
    shared = dict(input_ids=ids, attention_mask=am, patch_embeddings=b["patch_embeddings"], image_index=im)
    plain = dict(input_ids=ids, attention_mask=am, patch_embeddings=b["patch_embeddings"][im].contiguous())
    return shared, plain


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("case", list(DECODE_CASES))
def test_generate_shared_image_fp32_matches_reference_golden(case, use_cache):
    cfg, sd, batch, eos, max_new, tokens, step_logits, gaps = decode_setup(case)
    model = build_model(cfg, sd)
    shared, _ = _doubled(to_dev(batch))
    out, steps = model.generate(max_new_tokens=max_new, use_cache=use_cache, eos_token_id=eos, pad_token_id=eos, return_step_logits=True, **shared)
    want = tokens.repeat(2, 1)
    assert out.shape == want.shape, (out.shape, want.shape)
    assert torch.equal(out.cpu(), want), (out.cpu(), want)
    close(steps, step_logits.repeat(1, 2, 1), 1e-3, "last-position logits of every step")


def test_generate_shared_image_cross_pairing_equals_unshared():
    """Prompts and images paired across the fixture's rows: the shared prefill against the existing ``generate`` on
    ``patch_embeddings[image_index]``.  Logits are compared for as long as the two runs have produced the same tokens, tokens at the steps
    whose smallest top-2 gap (unshared run) is above 1e-2 x max|logit|; at least half of all steps must pass both comparisons."""
    compared = total = 0
    for case, images in [(c, im) for c in ("t64", "m64") for im in (CROSS_IMAGE, CROSS_IMAGE_2)]:
        cfg, sd, batch, eos, max_new, tokens, step_logits, gaps = decode_setup(case)
        model = build_model(cfg, sd)
        shared, plain = _crossed(to_dev(batch), images)
        kw = dict(max_new_tokens=max_new, use_cache=True, eos_token_id=eos, pad_token_id=eos, return_step_logits=True)
        out_s, st_s = model.generate(**shared, **kw)
        out_p, st_p = model.generate(**plain, **kw)
        T = shared["input_ids"].shape[1]
        n = out_p.shape[1] - T
        total += n
        assert out_s.shape[1] - T >= 1
        for i in range(min(n, out_s.shape[1] - T)):
            close(st_s[i], st_p[i], 1e-3, f"{case} step {i}: shared vs unshared logits")   # (step 0 always)
            top2 = st_p[i].topk(2, dim=-1).values
            gap = float((top2[:, 0] - top2[:, 1]).min())
            same = torch.equal(out_s[:, T + i], out_p[:, T + i])
            if gap > 1e-2 * float(st_p[i].abs().max()):
                assert same, f"{case} step {i}: tokens differ at a top-2 gap of {gap:.3e}"
                compared += 1
            if not same:
                break   # a near-tie flipped: later steps see different prefixes
    print(f"[cross] logits and tokens compared at {compared} of {total} steps")
    assert 2 * compared >= total, f"only {compared} of {total} steps compared"


@pytest.mark.parametrize("case", ["t64", "m64", "t128"])
def test_generate_shared_image_bf16_tracks_unshared(case):
    """bf16 (MFMA) mode: shared against unshared cached logits at bf16 level; the same tokens wherever the fp32 top-2 gap is far above
    bf16 noise (the rule of test_generate_bf16_cached_equals_uncached_and_tracks_fp32)."""
    cfg, sd, batch, eos, max_new, tokens, step_logits, gaps = decode_setup(case)
    model = build_model(cfg, sd, dtype=torch.bfloat16)
    shared, plain = _doubled(to_dev(batch), torch.bfloat16)
    kw = dict(max_new_tokens=max_new, eos_token_id=eos, return_step_logits=True, use_cache=True)
    out_s, st_s = model.generate(**shared, **kw)
    out_p, st_p = model.generate(**plain, **kw)
    T = shared["input_ids"].shape[1]
    scale = float(step_logits.abs().max())
    want = tokens.repeat(2, 1)
    for i in range(min(out_s.shape[1], out_p.shape[1]) - T):
        close(st_s[i], st_p[i], 3e-2, f"step {i}: shared vs unshared logits")
        if float(gaps[i].min()) < 0.05 * scale:
            break  # a near-tie may legitimately flip under bf16: later steps see different prefixes
        assert torch.equal(out_s[:, T + i], out_p[:, T + i]) and torch.equal(out_s[:, T + i].cpu(), want[:, T + i])


def test_beam_search_shared_image_equals_expanded_features():
    cfg, sd, batch, eos, max_new, *_ = decode_setup("t64")
    model = build_model(cfg, sd)
    shared, plain = _crossed(to_dev(batch))
    kw = dict(num_beams=3, num_return_sequences=3, max_new_tokens=max_new, eos_token_id=eos, pad_token_id=eos, use_cache=True,
              return_dict_in_generate=True)
    got, want = model.generate(**shared, **kw), model.generate(**plain, **kw)
    close(got.sequences_scores, want.sequences_scores, 1e-3, "sequences_scores")
    assert got.sequences.shape == want.sequences.shape
    # a returned hypothesis keeps its rank, hence its row, where its score is further than the bound from its returned neighbours'
    sc = want.sequences_scores.view(-1, 3).cpu()
    bound = 1e-3 * max(1.0, float(sc.abs().max()))
    far = (sc[:, :-1] - sc[:, 1:]).abs() > bound                          # [B, 2]: ranks j and j + 1 apart
    clear = torch.stack([far[:, 0], far[:, 0] & far[:, 1], far[:, 1]], dim=1).reshape(-1)
    print(f"[beam] scores {sc.tolist()}; bound {bound:.2e}; {int(clear.sum())} of {clear.numel()} hypotheses compared")
    clear = clear.to(DEV)
    assert torch.equal(got.sequences[clear], want.sequences[clear]), (got.sequences, want.sequences)
    # use_cache=False: the literal recompute on feats.index_select(0, image_index)
    kw["use_cache"] = False
    lit = model.generate(**shared, **kw)
    close(lit.sequences_scores, want.sequences_scores, 1e-3, "sequences_scores, recompute")


def test_sample_shared_image_equals_expanded_features():
    cfg, sd, batch, eos, max_new, *_ = decode_setup("t64")
    model = build_model(cfg, sd)
    shared, plain = _crossed(to_dev(batch))
    for n in (3, 1):
        kw = dict(num_return_sequences=n, seed=1234, max_new_tokens=max_new, eos_token_id=eos, pad_token_id=eos, use_cache=True,
                  return_logprobs=True, top_k=50)
        seq_s, lp_s = model.sample(**shared, **kw)
        seq_p, lp_p = model.sample(**plain, **kw)
        T = shared["input_ids"].shape[1]
        assert seq_s.shape[0] == 6 * n and torch.equal(seq_s[:, :T], seq_p[:, :T])
        assert torch.equal(seq_s[:, T], seq_p[:, T]), "the first step's tokens agree"
        for i in range(min(seq_s.shape[1], seq_p.shape[1]) - T):
            agree = seq_s[:, T + i] == seq_p[:, T + i]   # (rows still on the same path: a row that diverged once is dropped for good)
            if i == 0:
                alive = agree
            else:
                alive = alive & agree
            if not bool(alive.any()):
                break
            close(lp_s[alive, i], lp_p[alive, i], 1e-3, f"n = {n}, step {i}: log-probabilities of the drawn tokens")


def test_image_index_errors_and_the_untouched_path():
    cfg, sd, batch, eos, max_new, tokens, *_ = decode_setup("t64")
    model = build_model(cfg, sd)
    b = to_dev(batch)
    B = b["input_ids"].shape[0]
    kw = dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], max_new_tokens=2, eos_token_id=eos)
    feats = b["patch_embeddings"]
    assert "image_index" in inspect.signature(model.generate).parameters and "image_index" in inspect.signature(model.sample).parameters
    for fn in (model.generate, model.sample):
        for bad in (_idx([0] * (B + 1)), _idx([[0] * B]), torch.zeros(B, dtype=torch.int32, device=DEV), _idx([0] * (B - 1) + [B]),
                    _idx([-1] + [0] * (B - 1)), [0] * B):
            with pytest.raises(ValueError):
                fn(patch_embeddings=feats, image_index=bad, **kw)
        with pytest.raises(ValueError):   # N != B and no index to pair them
            fn(patch_embeddings=feats[:B - 1], **kw)
        with pytest.raises(NotImplementedError):
            fn(patch_embeddings=feats, image_index=_idx(list(range(B))), use_graph=True, **kw)
    with pytest.raises(ValueError):
        model.generate(patch_embeddings=feats, image_index=_idx([0] * B + [1]), num_beams=2, **kw)
    # no index: the existing path, the same tensor as ever
    full = dict(kw, max_new_tokens=max_new, patch_embeddings=feats, pad_token_id=eos)
    model.prefill_trace = []
    out1, out2 = model.generate(**full), model.generate(**full)
    assert torch.equal(out1, out2) and torch.equal(out1.cpu(), tokens) and model.prefill_trace == []
    # an index on the CPU, images as pixel_values features (class token in front): the same tokens
    pv = torch.cat([torch.zeros(B, 1, cfg.vision_hidden_size, device=DEV), feats], dim=1)
    out3 = model.generate(input_ids=b["input_ids"], attention_mask=b["attention_mask"], pixel_values=pv, max_new_tokens=max_new, eos_token_id=eos,
                          pad_token_id=eos, image_index=torch.arange(B))
    assert torch.equal(out3.cpu(), tokens) and len(model.prefill_trace) == 1


def test_shared_prefill_moves_each_image_through_the_stack_once():
    """N = 1, B = 4: P + B * T rows enter the first layer's QKV product (the rows of its two output stores), not B * (P + T)."""
    cfg, sd, batch, eos, max_new, *_ = decode_setup("t64")
    model = build_model(cfg, sd)
    b = to_dev(batch)
    t = _idx([0, 1, 2, 1])
    P, T, L, W = cfg.num_vision_tokens, b["input_ids"].shape[1], cfg.num_hidden_layers, 3 * cfg.hidden_size
    model.prefill_trace = []
    model.generate(input_ids=b["input_ids"][t].contiguous(), attention_mask=b["attention_mask"][t].contiguous(),
                   patch_embeddings=b["patch_embeddings"][1:2].contiguous(), image_index=_idx([0, 0, 0, 0]), max_new_tokens=2, eos_token_id=eos)
    assert len(model.prefill_trace) == 1
    tr = model.prefill_trace[0]
    assert tr["image_store"] == (L, P, W) and tr["text_store"] == (L, 4 * T, W) and tr["prefix"] == (L, 4 * (P + T), W)
    assert tr["image_store"][1] + tr["text_store"][1] == P + 4 * T
