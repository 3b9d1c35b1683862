"""CPU: the clip's side of the norm hand-over (``model.final_grad_sumsq``) -- which launch ``FlatAdamW.clip_grad_norm_`` makes with and
without handed-over partials -- with the ``ops`` functions replaced by recorders and a small real model on the CPU for the layout."""
import pytest
import torch


@pytest.fixture
def rig(monkeypatch):
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM, ops
    from mafed_amd.optim import FlatAdamW
    cfg = VLPythiaConfig(vocab_size=64, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                         vision_hidden_size=16, num_vision_tokens=4)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.float32, device="cpu")
    opt = FlatAdamW(model)
    calls = []

    def finish(partials, max_norm, out2, advance=None, norm_log=None):
        assert out2 is opt.clip_out
        calls.append(("gradnorm_finish", partials.data_ptr(), partials.numel(), advance is not None, norm_log is not None))

    def clip(g, max_norm, out2=None):
        assert out2 is opt.clip_out and g is model.flat_grads
        calls.append(("gradnorm_clip",))

    monkeypatch.setattr(ops, "gradnorm_finish", finish)
    monkeypatch.setattr(ops, "gradnorm_clip", clip)
    monkeypatch.setattr(ops, "optim_advance_", lambda *a, **k: calls.append(("optim_advance_",)))
    return model, opt, calls


@pytest.mark.parametrize("fuse_advance", [False, True])
def test_handed_over_partials_are_folded_once(rig, fuse_advance):
    model, opt, calls = rig
    assert model.final_grad_sumsq is None
    handed = model.final_grad_sumsq = torch.zeros(5)
    out = opt.clip_grad_norm_(2.0, fuse_advance=fuse_advance)
    assert calls == [("gradnorm_finish", handed.data_ptr(), 5, fuse_advance, fuse_advance)]
    assert model.final_grad_sumsq is None and opt.advance_fused == fuse_advance
    # fused: the norm sits in a log slot of its own; else in clip_out[0]
    assert (out.data_ptr() == opt.clip_out.data_ptr()) == (not fuse_advance)
    opt.advance()   # (the fused finish has advanced the schedule: nothing launched; else the guarded advance)
    assert calls[1:] == ([] if fuse_advance else [("optim_advance_",)])
    # used up: the next clip reads the buffer, exactly as before
    del calls[:]
    opt.clip_grad_norm_(2.0, fuse_advance=fuse_advance)
    assert calls == [("gradnorm_clip",)]


def test_zero_grad_drops_a_hand_over(rig):
    model, opt, calls = rig
    model.final_grad_sumsq = torch.zeros(5)
    model.zero_grad()
    assert model.final_grad_sumsq is None
    opt.clip_grad_norm_(2.0)
    assert calls == [("gradnorm_clip",)]


def test_hand_over_without_the_flat_layer_layout(rig):
    """A model for which the optimiser keeps no incremental norm: the partials are folded by a plain finish."""
    model, opt, calls = rig
    opt.norm = None
    handed = model.final_grad_sumsq = torch.zeros(3)
    out = opt.clip_grad_norm_(2.0, fuse_advance=True)
    assert calls == [("gradnorm_finish", handed.data_ptr(), 3, False, False)]
    assert model.final_grad_sumsq is None and not opt.advance_fused and out.data_ptr() == opt.clip_out.data_ptr()
