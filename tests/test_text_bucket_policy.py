"""CPU: the ``text_bucket`` policy (mafed_amd.model.bucket_text_len) -- which text length T' a [B, T] batch with P image positions runs
at.  "auto" takes the smallest T' >= T with B * (P + T') a multiple of 128 when that costs at most 16 positions per sample, and leaves
the batch alone otherwise; an int m takes (P + T') to a multiple of m; 0 is off.  No GPU, no kernels."""
import copy

import pytest
import torch

from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
from mafed_amd.model import TEXT_BUCKET_MAX_PAD, TEXT_BUCKET_ROWS, bucket_text_len

AUTO = [
    # B, P, T -> T'
    (16, 256, 23, 24), (16, 256, 24, 24), (16, 256, 29, 32), (16, 256, 32, 32), (16, 256, 17, 24), (16, 256, 60, 64), (16, 104, 23, 24),
    (32, 256, 23, 24), (32, 256, 24, 24), (32, 256, 25, 28), (32, 256, 29, 32), (32, 256, 30, 32), (32, 256, 32, 32),
    # an odd B needs P + T' itself to be a multiple of 128: out of reach for a question, left alone
    (13, 256, 23, 23), (13, 256, 32, 32), (1, 256, 23, 23), (1, 256, 60, 60),
    # ... unless it happens to be near
    (13, 256, 120, 128), (1, 256, 127, 128), (1, 256, 128, 128),
]


@pytest.mark.parametrize("B,P,T,want", AUTO)
def test_auto_table(B, P, T, want):
    got = bucket_text_len("auto", B, P, T)
    assert got == want
    assert got == T or (B * (P + got)) % TEXT_BUCKET_ROWS == 0
    assert bucket_text_len("auto", B, P, got) == got, "a batch at the padded length stays there"


def test_auto_cap_is_sixteen_positions():
    assert TEXT_BUCKET_MAX_PAD == 16 and TEXT_BUCKET_ROWS == 128
    # B = 8: P + T' a multiple of 16 -- never more than 15 away
    assert bucket_text_len("auto", 8, 256, 1) == 16
    # B = 4: P + T' a multiple of 32
    assert bucket_text_len("auto", 4, 256, 16) == 32      # 16 positions: the cap itself
    assert bucket_text_len("auto", 4, 256, 15) == 15      # 17 positions: over the cap, not padded
    assert bucket_text_len("auto", 4, 256, 1) == 1
    for B in (1, 2, 4, 8, 13, 16, 32, 48):
        for T in range(1, 70):
            Tp = bucket_text_len("auto", B, 256, T)
            assert T <= Tp <= T + 16
            if Tp == T and (B * (256 + T)) % 128:
                assert all((B * (256 + t)) % 128 for t in range(T, T + 17)), (B, T)


def test_int_and_off():
    assert bucket_text_len(8, 3, 8, 6) == 8            # the golden configurations: S = 14 -> 16
    assert bucket_text_len(8, 3, 8, 7) == 8
    assert bucket_text_len(8, 3, 40, 24) == 24         # S = 64 already
    assert bucket_text_len(64, 5, 256, 23) == 64       # an int does not look at B
    for off in (0, None, False):
        assert bucket_text_len(off, 16, 256, 23) == 23
    for bad in ("on", -8):
        with pytest.raises(ValueError):
            bucket_text_len(bad, 16, 256, 23)


def test_model_defaults_attribute_and_teacher_copy():
    cfg = VLPythiaConfig(vocab_size=64, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                         vision_hidden_size=16, num_vision_tokens=8)
    m32 = VLPythiaForCausalLM(cfg, compute_dtype=torch.float32, device="cpu")
    assert m32.text_bucket == 0, "fp32 mode: the exact kernels take any shape, nothing is appended unless asked for"
    assert m32.padded_text_len(3, 6) == 6
    mbf = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device="cpu")
    assert mbf.text_bucket == "auto"
    assert mbf.padded_text_len(16, 23) == 24           # P = 8: S = 31 -> 32
    m32.text_bucket = 8                                 # settable as an attribute
    assert m32.padded_text_len(3, 6) == 8
    assert copy.deepcopy(m32).text_bucket == 8          # the frozen teacher runs the same policy
    assert VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device="cpu", text_bucket=0).padded_text_len(16, 23) == 23
    with pytest.raises(ValueError):
        VLPythiaForCausalLM(cfg, compute_dtype=torch.float32, device="cpu", text_bucket="yes")
