"""CPU guard of the whole-step parity bounds (tests/helpers.py: STEP_RTOL, STEP_RTOL_BF16, UPDATE_RTOL): the fp64 oracle against
deliberately mutated fp64 oracles must be rejected by the exact comparators and constants that tests/test_gpu_model.py applies to
the native step, each by at least GUARD_MARGIN times its bound, on every case the GPU tests run.  Loosening a bound past what these
mutations change fails here."""
import dataclasses
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import vlpythia_ref as R
from tests.helpers import (GUARD_MARGIN, STEP_CASES, STEP_RTOL, STEP_RTOL_BF16, TINY, TRAINER_CASE, UPDATE_RTOL, check_step_parity,
                           check_updates, step_case, step_fp64, step_parity_errors, step_ref, tiny_cfg, trainer_fp64,
                           update_errors)

STEP_MUTATIONS = ("tanh_gelu", "rotary_base_10500", "ln_eps_1e-6", "key_padding_ignored", "label_dropped", "rotary_pct_0.5")
BF16_MUTATIONS = ("key_padding_ignored", "label_dropped")


class _TanhGelu(types.ModuleType):
    """torch.nn.functional with gelu replaced by its tanh approximation."""

    def __init__(self):
        super().__init__("functional_tanh_gelu")

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def gelu(x):
        return F.gelu(x, approximate="tanh")


def _drop_one_label(batch):
    """The last label of the first sample that has one (a position the shifted CE reads) set to -100."""
    b = dict(batch)
    labels = batch["labels"].clone()
    row = next(i for i in range(labels.shape[0]) if int(labels[i, -1]) != -100)
    labels[row, -1] = -100
    b["labels"] = labels
    return b


def mutated_step(name, mutation, monkeypatch):
    cfg, sd, batch = step_case(name)
    with monkeypatch.context() as mp:
        if mutation == "tanh_gelu":
            mp.setattr(R, "F", _TanhGelu())
        elif mutation == "rotary_base_10500":
            cfg = dataclasses.replace(cfg, rotary_emb_base=10500.0)
        elif mutation == "ln_eps_1e-6":
            cfg = dataclasses.replace(cfg, layer_norm_eps=1e-6)
        elif mutation == "key_padding_ignored":
            real = R.additive_mask
            mp.setattr(R, "additive_mask", lambda am: real(torch.ones_like(am)))
        elif mutation == "label_dropped":
            batch = _drop_one_label(batch)
        elif mutation == "rotary_pct_0.5":
            cfg = dataclasses.replace(cfg, rotary_pct=0.5)
        else:
            raise KeyError(mutation)
        return step_fp64(cfg, sd, batch)


def assert_step_rejected(mut, ref, rtol, what, without_logits=False):
    if without_logits:
        mut = {k: v for k, v in mut.items() if k != "logits"}
    errs = step_parity_errors(mut, ref)
    worst = max(errs.values())
    print(f"[guard] {what}: largest change {worst:.3e} ({worst / rtol:.1f} x bound {rtol:.1e})")
    assert worst > GUARD_MARGIN * rtol, f"{what}: mutation moves nothing by more than {worst:.3e} (bound {rtol:.1e})"
    with pytest.raises(AssertionError):
        check_step_parity(mut, ref, rtol, what)


@pytest.mark.parametrize("name", STEP_CASES)
def test_step_bound_rejects_mutations(name, monkeypatch):
    """test_forward_backward_vs_fp64_oracle (STEP_RTOL): every mutation on every case it runs; the second, accumulated backward
    goes through the same comparator (grad_mul = 2), where a mutated gradient is off by the same relative amount."""
    ref = step_ref(name)
    assert check_step_parity(ref, ref, STEP_RTOL, f"{name}/unmutated") == 0.0
    for m in STEP_MUTATIONS:
        mut = mutated_step(name, m, monkeypatch)
        assert_step_rejected(mut, ref, STEP_RTOL, f"{name}/{m}")
        twice = dict(mut, grads={k: 2 * v for k, v in mut["grads"].items()})
        gerr = {k: v for k, v in step_parity_errors(twice, ref, grad_mul=2.0).items() if k.startswith("grad")}
        assert max(gerr.values()) > GUARD_MARGIN * STEP_RTOL, (name, m, max(gerr.values()))


@pytest.mark.parametrize("name", list(TINY))
def test_bf16_step_bound_rejects_mutations(name, monkeypatch):
    """test_bf16_step_vs_fp64_oracle (STEP_RTOL_BF16; loss, hidden states and gradients, no logits): ignored key padding and the
    dropped label are rejected.  The tanh GELU (at most 3e-4 of a tensor on these configs), the rotary base (7e-4), the LayerNorm
    eps (1.2e-2) and rotary_pct 0.5 (4.5e-2) are below what a bf16 step, whose rounding alone moves a gradient tensor by about 1 %,
    can resolve with a margin; they are left to the fp32 check."""
    ref = step_ref(name)
    for m in BF16_MUTATIONS:
        assert_step_rejected(mutated_step(name, m, monkeypatch), ref, STEP_RTOL_BF16, f"{name}/bf16/{m}", without_logits=True)


_TRAINER_REF = {}


def trainer_ref():
    if not _TRAINER_REF:
        _TRAINER_REF.update(trainer_fp64())
    return _TRAINER_REF


UPDATE_MUTATIONS = {"eps_1e-8": dict(eps=1e-8), "beta2_0.999": dict(betas=(0.9, 0.999)), "clip_2.2": dict(grad_clip=2.2),
                    "weight_decay_0.02": dict(weight_decay=0.02)}


@pytest.mark.parametrize("mutation", list(UPDATE_MUTATIONS))
def test_update_bound_rejects_mutations(mutation):
    """test_trainer_updates_vs_fp64_oracle (UPDATE_RTOL on final - initial of every parameter tensor): AdamW eps 1e-8, beta2 0.999,
    the clip at 2.2 and weight decay 0.02."""
    ref = trainer_ref()
    H = tiny_cfg(TRAINER_CASE["name"]).num_attention_heads
    assert ref["lr"][0] == 0.0 and (ref["lr"][1:] > 0).all() and len(ref["lr"]) == 8
    assert (ref["grad_norm"] > 2.2).any(), "the clip must bind for its mutation to mean anything"
    mut = trainer_fp64(**UPDATE_MUTATIONS[mutation])
    errs = update_errors(mut["update"], ref["update"], H)
    worst = max(errs.values())
    print(f"[guard] {mutation}: largest change {worst:.3e} ({worst / UPDATE_RTOL:.1f} x bound {UPDATE_RTOL:.1e}), "
          f"{sum(v > GUARD_MARGIN * UPDATE_RTOL for v in errs.values())} of {len(errs)} tensors")
    assert worst > GUARD_MARGIN * UPDATE_RTOL, f"{mutation}: moves no update by more than {worst:.3e} (bound {UPDATE_RTOL:.1e})"
    with pytest.raises(AssertionError):
        check_updates(mut["update"], ref["update"], UPDATE_RTOL, H, mutation)


def test_comparators_on_an_exactly_zero_reference():
    """A reference tensor that is exactly zero (a parameter the loss does not reach) must come out exactly zero, under any bound;
    and each comparator gives exactly zero on its own reference."""
    ref = step_ref("t64")
    k = "vision_embed_tokens.2.bias"
    zero = dict(ref, grads=dict(ref["grads"], **{k: torch.zeros_like(ref["grads"][k])}))
    assert check_step_parity(zero, zero, STEP_RTOL, "zero reference") == 0.0
    tiny = dict(zero, grads=dict(zero["grads"], **{k: torch.full_like(ref["grads"][k], 1e-30)}))
    with pytest.raises(AssertionError, match=k):
        check_step_parity(tiny, zero, 1.0, "zero reference, got 1e-30")
    upd = trainer_ref()["update"]
    H = tiny_cfg(TRAINER_CASE["name"]).num_attention_heads
    assert check_updates(upd, upd, UPDATE_RTOL, H, "unmutated") == 0.0
    with pytest.raises(AssertionError, match=k):
        check_updates(dict(upd, **{k: torch.full_like(upd[k], 1e-30)}), dict(upd, **{k: torch.zeros_like(upd[k])}), 1.0, H, "zero update")
