"""CPU restatement of ``model.score`` on the oracle, shared by tools/gen_score_golden.py and the scoring tests: the B * C expanded
sequences [image | prompt | candidate] through ``oracle.vlpythia_ref.forward``, ``log_softmax`` of the rows that predict the candidate
tokens, masked sums and means.  It does not import the product."""
import torch

from oracle import vlpythia_ref as R
from tests.helpers import TINY, load_golden, tiny_cfg

SCORE_CASES = ("t64", "m64", "t128", "t256")
C, A = 5, 4
GAP = 1e-2   # a prompt's ranking is compared when its top-2 score gap exceeds GAP x max|finite score| of its case


def score_setup(case):
    """(cfg, weights, batch) of the decode fixture's model ``case``: what ``tests.helpers.decode_setup`` builds for its cases (t256 has
    no decode case of its own; the recipe is the same)."""
    seed = int(load_golden("decode.npz")["seed"])
    cfg, t = tiny_cfg(case), TINY[case]
    sd = R.init_weights(cfg, seed=seed)
    return cfg, sd, R.make_batch(cfg, t["B"], t["T"], seed=seed + 1, pad=True)


def expand(batch, cand, mask):
    """The B * C sequences [prompt | candidate] (masked candidate positions hold token 0 and are attended: they come last)."""
    B, Cn, An = cand.shape
    tok = cand * (mask != 0)
    return {"input_ids": torch.cat([batch["input_ids"].repeat_interleave(Cn, 0), tok.view(B * Cn, An)], dim=1),
            "attention_mask": torch.cat([batch["attention_mask"].repeat_interleave(Cn, 0), torch.ones(B * Cn, An, dtype=torch.int64)], dim=1),
            "patch_embeddings": batch["patch_embeddings"].repeat_interleave(Cn, 0)}


def score_ref(sd, cfg, batch, cand, mask):
    """-> (token log-probabilities fp32 [B, C, A], 0 at masked positions; score_sum [B, C]; score_mean [B, C]; -inf without a token)."""
    B, Cn, An = cand.shape
    keep = mask != 0
    with torch.no_grad():
        logits = R.forward(sd, expand(batch, cand, mask), cfg).logits   # [B*C, P+T+A, V]
    lp = torch.log_softmax(logits[:, -(An + 1):-1, :].float(), dim=-1)   # position S0 - 1 + j predicts candidate token j
    tlp = lp.gather(-1, (cand * keep).view(B * Cn, An, 1)).view(B, Cn, An)
    tlp = torch.where(keep, tlp, torch.zeros_like(tlp))
    n = keep.sum(-1)
    ninf = torch.full((B, Cn), float("-inf"))
    ssum = torch.where(n > 0, tlp.sum(-1), ninf)
    return tlp, ssum, torch.where(n > 0, ssum / n.clamp(min=1), ninf)


def labelled_batch(batch, cand, mask, gold):
    """The fixture batch with candidate ``gold[b]`` of every prompt appended as its labelled answer: text [question | answer], labels -100
    outside the answer's tokens."""
    B = cand.shape[0]
    ar = torch.arange(B)
    ans, am = cand[ar, gold], mask[ar, gold]
    return {"input_ids": torch.cat([batch["input_ids"], ans * (am != 0)], dim=1),
            "attention_mask": torch.cat([batch["attention_mask"], am], dim=1),
            "labels": torch.cat([torch.full_like(batch["input_ids"], -100), torch.where(am != 0, ans, torch.full_like(ans, -100))], dim=1),
            "patch_embeddings": batch["patch_embeddings"]}


def ranked_prompts(score):
    """bool [B]: the prompts whose two best finite scores lie further apart than GAP x max|finite score| of the whole case."""
    finite = torch.isfinite(score)
    scale = float(score[finite].abs().max())
    top2 = torch.where(finite, score, torch.full_like(score, -1e30)).topk(2, dim=-1).values
    return (top2[:, 0] - top2[:, 1]) > GAP * scale
