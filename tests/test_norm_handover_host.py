"""CPU: which launches the optimiser makes around a backward sweep -- the incremental clip norm (hook partials, finish, the one-pass
fall-back) and the chunked AdamW pass -- driven only through ``begin_incremental_norm``, the hook it returns, ``clip_grad_norm_``,
``advance`` and ``apply``, with the ``ops`` functions replaced by recorders and a small real model on the CPU for the layout."""
import pytest
import torch


def _sweep(model, filled=False):
    """What a backward sweep leaves on the model before its first gradient hook fires: the next serial, and whether its weight-gradient
    GEMMs fill ``dw_sumsq``.  (The only place of this file that writes the sweep's record by hand.)"""
    from mafed_amd.model import SweepRecord
    model.last_sweep = SweepRecord(model.last_sweep.serial + 1, filled_squares=bool(filled and model.dw_sumsq is not None))


L, H = 3, 32


@pytest.fixture
def rig(monkeypatch):
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM, ops
    from mafed_amd.dist import layer_ranges
    from mafed_amd.optim import FlatAdamW
    cfg = VLPythiaConfig(vocab_size=64, hidden_size=H, num_hidden_layers=L, num_attention_heads=2, intermediate_size=4 * H,
                         vision_hidden_size=16, num_vision_tokens=4)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.float32, device="cpu")
    opt = FlatAdamW(model, weight_decay=0.01)
    calls = []

    def off(t, base):
        return t.storage_offset() - base.storage_offset()

    def partial(g, part):
        lo = off(g, model.flat_grads)
        calls.append(("gradnorm_partial", lo, lo + g.numel(), part.storage_offset()))

    def finish(partials, max_norm, out2, advance=None, norm_log=None):
        assert out2 is opt.clip_out and partials.storage_offset() == 0
        calls.append(("gradnorm_finish", partials.numel(), advance is not None, norm_log is not None))

    def clip(g, max_norm, out2=None):
        assert out2 is opt.clip_out
        calls.append(("gradnorm_clip", off(g, model.flat_grads), off(g, model.flat_grads) + g.numel()))

    def advance(state, *a, clip=None):
        calls.append(("optim_advance_", clip is not None))

    def adamw(p, g, m, v, lr_dev, b1, b2, eps, wd, step, clip=None, grad_mul=1.0, p_bf16=None, zero_grad=False, zero_n=None):
        lo = off(p, model.flat_params)
        assert off(g, model.flat_grads) == lo and g.numel() == p.numel()
        calls.append(("adamw_step_", lo, lo + p.numel(), wd, clip is not None, zero_grad, zero_n))

    for name, fn in (("gradnorm_partial", partial), ("gradnorm_finish", finish), ("gradnorm_clip", clip), ("optim_advance_", advance),
                     ("adamw_step_", adamw)):
        monkeypatch.setattr(ops, name, fn)
    per_layer, head, tail = layer_ranges(model)
    # (trigger, lo, hi) in the order a sweep finishes the ranges, and each range's first partial slot
    order = [(L,) + tuple(head)] + [(i,) + tuple(per_layer[i]) for i in range(L - 1, -1, -1)] + [(-1,) + tuple(r) for r in tail]
    slots, s = [], 0
    for _, lo, hi in order:
        slots.append(s)
        s += ops.gradnorm_blocks(hi - lo)
    n_partials = s + 16 * 4 * L
    return model, opt, calls, order, slots, n_partials


def _report(hook, which):
    for i in which:
        hook(i)


ALL = [L] + list(range(L - 1, -1, -1)) + [-1]


def _whole_ranges(order, slots):
    return [("gradnorm_partial", lo, hi, s) for (_, lo, hi), s in zip(order, slots)]


@pytest.mark.parametrize("fuse_advance", [False, True])
def test_every_range_reported_in_the_last_sweep_finishes_from_the_partials(rig, fuse_advance):
    model, opt, calls, order, slots, n_partials = rig
    hook = opt.begin_incremental_norm()
    assert hook is not None and model.dw_sumsq is None
    _sweep(model)
    _report(hook, ALL)
    assert calls == _whole_ranges(order, slots)
    calls.clear()
    gn = opt.clip_grad_norm_(2.0, fuse_advance=fuse_advance)
    assert calls == [("gradnorm_finish", n_partials, fuse_advance, fuse_advance)]   # no pass over the buffer
    assert gn.numel() == 1 and (gn.data_ptr() == opt.clip_out.data_ptr()) == (not fuse_advance)
    calls.clear()
    opt.advance()
    assert calls == ([] if fuse_advance else [("optim_advance_", True)])
    calls.clear()
    opt.advance()   # (the next step's: the fused advance covered one step only; no clip pending -> unguarded only after apply)
    assert calls == [("optim_advance_", True)]
    opt.apply()
    calls.clear()
    opt.advance()
    assert calls == [("optim_advance_", False)]


def test_a_range_that_never_reports_gives_the_one_pass_norm(rig):
    model, opt, calls, order, slots, _ = rig
    hook = opt.begin_incremental_norm()
    _sweep(model)
    _report(hook, [i for i in ALL if i != 1])
    calls.clear()
    gn = opt.clip_grad_norm_(2.0, fuse_advance=True)
    assert calls == [("gradnorm_clip", 0, model.flat_grads.numel())]
    assert gn.data_ptr() == opt.clip_out.data_ptr()
    calls.clear()
    opt.advance()
    assert calls == [("optim_advance_", True)]


def test_a_further_sweep_before_the_clip_gives_the_one_pass_norm(rig):
    model, opt, calls, order, slots, _ = rig
    hook = opt.begin_incremental_norm()
    _sweep(model)
    _report(hook, ALL)
    _sweep(model)   # (a plugin's extra backward whose hooks did not all fire: the partials are one sweep old)
    _report(hook, [L])
    calls.clear()
    opt.clip_grad_norm_(2.0)
    assert calls == [("gradnorm_clip", 0, model.flat_grads.numel())]


def test_the_hook_may_fire_after_the_clip_consumed_the_record(rig):
    model, opt, calls, order, slots, n_partials = rig
    hook = opt.begin_incremental_norm()
    _sweep(model)
    _report(hook, ALL)
    opt.clip_grad_norm_(2.0)
    calls.clear()
    _sweep(model)   # a backward outside the step while the hook is still installed
    _report(hook, ALL)
    assert calls == _whole_ranges(order, slots)
    # the next armed window is unaffected: complete -> finish, incomplete -> one pass
    hook = opt.begin_incremental_norm()
    _sweep(model)
    _report(hook, ALL)
    calls.clear()
    opt.clip_grad_norm_(2.0)
    assert calls == [("gradnorm_finish", n_partials, False, False)]
    hook = opt.begin_incremental_norm()
    _sweep(model)
    _report(hook, ALL[:-1])
    calls.clear()
    opt.clip_grad_norm_(2.0)
    assert calls == [("gradnorm_clip", 0, model.flat_grads.numel())]


@pytest.mark.parametrize("filled", [True, False])
def test_fused_squares_shorten_a_layer_range_only_when_the_sweep_filled_them(rig, filled):
    model, opt, calls, order, slots, n_partials = rig
    hook = opt.begin_incremental_norm(fused_matrix_squares=True)
    sq = model.dw_sumsq
    assert sq is not None and tuple(sq.shape) == (L, 4, 16) and sq.storage_offset() == n_partials - 16 * 4 * L
    _sweep(model, filled=filled)
    _report(hook, ALL)
    want = []
    for (t, lo, hi), s in zip(order, slots):
        if filled and 0 <= t < L:
            hi = model.layer_matrix_range(t)[0]   # the LayerNorm weights only
            assert lo < hi
        want.append(("gradnorm_partial", lo, hi, s))
    assert calls == want
    calls.clear()
    opt.clip_grad_norm_(2.0)
    assert calls == [("gradnorm_finish", n_partials, False, False)]


def test_apply_with_the_matrices_left_to_the_next_sweep(rig):
    model, opt, calls, order, slots, _ = rig
    opt.clip_grad_norm_(2.0)
    calls.clear()
    assert not model._dw_stale
    opt.apply(grad_mul=0.5, zero_grads=True, skip_matrix_zero=True)
    chunks = opt._chunks()
    assert [c[0] for c in chunks] == ["pre"] * 3 + [("layer", i) for i in range(L)] + ["head"]
    want = []
    for key, lo, hi, wd in chunks:
        zn = model.layer_matrix_range(key[1])[0] - lo if isinstance(key, tuple) else None
        want.append(("adamw_step_", lo, hi, wd, True, True, zn))
    assert calls == want and all(c[6] == 2 * 64 for c in calls if c[6] is not None)
    assert model._dw_stale
    # the clip scale is consumed by that pass; the plain pass is one launch per weight-decay segment and leaves the flag alone
    model._dw_stale = False
    calls.clear()
    opt.apply(zero_grads=True)
    n_decay = model.decay_split()
    assert calls == [("adamw_step_", 0, n_decay, 0.01, False, True, None),
                     ("adamw_step_", n_decay, model.flat_grads.numel(), 0.0, False, True, None)]
    assert not model._dw_stale
