"""GPU: the teacher cache read in place by the distillation kernels (``ops.TeacherRows``), in fp32 or bf16
(``FeatureDistillation(teacher_cache_dtype=...)`` / ``build_teacher_cache(dtype=...)``).  Config m64, fp32 compute, four
``Trainer.step``s per run, after tests/test_gpu_replay.py::test_teacher_cache_steps_are_bit_identical_to_the_teacher_forward.

The bounds are that test's: the first step's loss and gradient norm equal as floats (same weights, same batch, same teacher bits);
every step within 1e-6 relative loss and 1e-5 relative norm, the final parameters within 1e-6 absolute -- the run-to-run noise of
the backward's fp32 atomics.  A bf16 cache is compared with an UNCACHED run whose teacher forward returns ``x.bfloat16().float()``:
the kernels widen bf16 exactly, so the two runs feed the same numbers to the same arithmetic.
"""
import types

import pytest
import torch

from oracle import vlpythia_ref as R
from tests.helpers import TINY, tiny_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(cfg, sd, dtype=torch.float32):
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    mc = VLPythiaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        vision_hidden_size=cfg.vision_hidden_size, num_vision_tokens=cfg.num_vision_tokens)
    m = VLPythiaForCausalLM(mc, compute_dtype=dtype, device=DEV)
    m.load_state_dict(sd, strict=True)
    return m


def _conf():
    return types.SimpleNamespace(accumulate_grad_batches=1, replay_interval=1, grad_norm=2.0, learning_rate=1e-3, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_steps=0, total_steps=100)


_SETUP = {}


def _setup():
    if not _SETUP:
        cfg, t = tiny_cfg("m64"), TINY["m64"]
        B, T = t["B"], t["T"]
        n_mem = 5 * B + 3                       # a ragged tail: the fill re-runs the last full batch
        sd = R.init_weights(cfg, seed=31, bias_std=0.02, ln_jitter=0.05)
        tsd = R.perturb(sd, seed=32, std=5e-3)
        data = R.make_batch(cfg, n_mem, T, seed=33, pad=True, n_answer=3)
        data["patch_embeddings"] = data["patch_embeddings"].to(torch.bfloat16).float()   # the buffer stores bf16 features
        _SETUP.update(cfg=cfg, B=B, T=T, sd=sd, tsd=tsd, data=data)
    return _SETUP


def _make(rank=0, world=1, **fd_kw):
    from mafed_amd import FeatureDistillation
    from mafed_amd.methods import HBMReplayBuffer
    s = _setup()
    cfg, B = s["cfg"], s["B"]
    attrs = {k: fd_kw.pop(k) for k in ("fused_distill", "overlap_teacher") if k in fd_kw}
    model, teacher = _model(cfg, s["sd"]), _model(cfg, s["tsd"])
    opts = types.SimpleNamespace(tasks=["a", "b"], batch_size=B, seed=3, pin_mem=False, accumulate_grad_batches=1)
    fd = FeatureDistillation(memory_size=10, opts=opts, model_type="vlpythia", num_hidden_layers=cfg.num_hidden_layers - 1,
                             distillation_modality_weighing_strategy="balanced", distillation_layer_weighing_strategy="discounted",
                             gamma=0.5, distillation_layer=None, **fd_kw)
    for k, v in attrs.items():
        setattr(fd, k, v)
    fd._update_model(teacher)
    fd.task_id = 1
    fd.num_vision_tokens = cfg.num_vision_tokens
    mem = HBMReplayBuffer(B, DEV, seed=9, rank=rank, world_size=world)
    mem.add(s["data"])
    fd.mem_dataloader = mem
    return fd, model, mem


def _steps(fd, model, cache, round_teacher=False):
    """Four optimiser steps -> (losses, gradient norms, parameters).  ``cache``: None, or the dtype of a teacher cache built first; then
    the teacher forward must not run, no gather may read the cache, and every consumer must have been handed TeacherRows."""
    from mafed_amd import Trainer, ops
    s = _setup()
    orig = fd.past_model.hidden_states_upto
    forwards, gathers, seen = [], [], []
    if cache is not None:
        fd.build_teacher_cache(dtype=cache)
        assert fd._tcache["states"].dtype == cache
        storage = fd._tcache["states"].untyped_storage().data_ptr()
        fd.past_model.hidden_states_upto = lambda *a, **k: (forwards.append(1), orig(*a, **k))[1]
    elif round_teacher:
        fd.past_model.hidden_states_upto = lambda *a, **k: [x.bfloat16().float() for x in orig(*a, **k)]
    gather = ops.gather_rows
    ops.gather_rows = lambda src, idx: (gathers.append(src.untyped_storage().data_ptr()), gather(src, idx))[1]
    rows_of = fd._teacher_rows
    fd._teacher_rows = lambda *a, **k: (lambda hs: (seen.append(hs is not None), hs)[1])(rows_of(*a, **k))
    try:
        tr = Trainer(model, fd, _conf(), task_id=1, pipeline_optimizer=True)
        task = {k: v[:s["B"]].to(DEV) for k, v in s["data"].items()}
        losses, gns = [], []
        for i in range(4):
            rec = tr.step(task, i)
            assert rec["branch"] == "replay" and rec["stepped"]
            losses.append(rec["loss"]); gns.append(rec["grad_norm"])
        tr.join()
        torch.cuda.synchronize()
    finally:
        ops.gather_rows = gather
    if cache is not None:
        assert not forwards, "the teacher forward ran although its states are cached"
        assert storage not in gathers, "a replay step gathered a copy of the cached teacher rows"
        assert seen == [True] * 4, seen           # once per step, every time the in-place rows
    return [float(x) for x in losses], [float(x) for x in gns], model.flat_params.clone()


def _compare(a, b):
    (la, ga, pa), (lb, gb, pb) = a, b
    print("loss", la, lb, "norm", ga, gb, "max |dp|", float((pa - pb).abs().max()))
    assert la[0] == lb[0] and ga[0] == gb[0], (la, lb, ga, gb)     # same weights, same batch, same teacher bits
    assert all(abs(x - y) <= 1e-6 * abs(x) for x, y in zip(la, lb)), (la, lb)
    assert all(abs(x - y) <= 1e-5 * abs(x) for x, y in zip(ga, gb)), (ga, gb)
    assert float((pa - pb).abs().max()) <= 1e-6
    assert len(set(la)) == 4


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_fp32_cache_read_in_place_matches_the_teacher_forward(rank, world):
    fd0, m0, _ = _make(rank, world)
    ref = _steps(fd0, m0, None)
    fd1, m1, mem = _make(rank, world)
    got = _steps(fd1, m1, torch.float32)
    _compare(got, ref)
    assert mem.attach_index
    fd1._update_model(m1)
    assert fd1._tcache is None and not mem.attach_index, "a new teacher must drop the cached states"


VARIANTS = {"mse": dict(distillation_loss="mse"), "cosine": dict(distillation_loss="cosine"),
            "cls": dict(distillation_loss="cosine", cls_distillation=True)}


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_bf16_cache_matches_an_uncached_run_with_the_rounded_teacher(variant, fused, overlap):
    kw = dict(VARIANTS[variant], fused_distill=fused, overlap_teacher=overlap)
    fd0, m0, _ = _make(**kw)
    ref = _steps(fd0, m0, None, round_teacher=True)
    fd1, m1, mem = _make(teacher_cache_dtype="bf16", **kw)
    assert fd1.teacher_cache_dtype == torch.bfloat16
    got = _steps(fd1, m1, fd1.teacher_cache_dtype)
    _compare(got, ref)
    fd1._update_model(m1)
    assert fd1._tcache is None and not mem.attach_index


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_bf16_cache_contents_size_and_dense_accessor(rank, world):
    s = _setup()
    B = s["B"]
    fd32, _, _ = _make(rank, world)
    gb32 = fd32.build_teacher_cache()["GB"]
    assert fd32._tcache["states"].dtype == torch.float32
    fd32.drop_teacher_cache()
    fd, _, mem = _make(rank, world, teacher_cache_dtype=torch.bfloat16)
    info = fd.build_teacher_cache()
    lo, hi = mem.shard()
    states = fd._tcache["states"]
    assert states.dtype == torch.bfloat16 and info["samples"] == hi - lo
    assert info["GB"] == gb32 / 2 == states.numel() * 2 / 1e9
    layers = fd.loss_weights.get_distillation_layers()
    for idx in (torch.arange(lo, lo + B), torch.arange(hi - B, hi), torch.tensor([lo, hi - 1, lo + 7, lo + B, lo + 2 * B + 1, lo + 3, hi - 2, lo + 11][:B])):
        idx = idx.to(DEV)
        want = fd.past_model.hidden_states_upto(mem.data["input_ids"][idx], mem.data["attention_mask"][idx],
                                                patch_embeddings=mem.data["patch_embeddings"][idx], n_hidden=max(layers) + 1)
        fd._mem_index = idx
        dense = fd._cached_teacher_states(max(layers) + 1)
        rows = fd._teacher_rows(max(layers) + 1)
        for k, l in enumerate(layers):
            w16 = want[l].view(B, -1, states.shape[-1]).bfloat16()
            assert torch.equal(states[k][idx - lo], w16), f"cached bf16 state of layer {l} is not the forward's state rounded"
            assert dense[l].dtype == torch.float32 and torch.equal(dense[l], w16.float())
            assert rows[l].states.data_ptr() == states[k].data_ptr() and rows[l].index.dtype == torch.int32
            assert torch.equal(rows[l].index.long(), idx - lo) and torch.equal(rows[l].materialize(), dense[l])
    fd._mem_index = None


def test_cache_dtype_interface():
    from mafed_amd import FeatureDistillation
    opts = types.SimpleNamespace(tasks=["a", "b"], batch_size=3, seed=3, pin_mem=False, accumulate_grad_batches=1)
    kw = dict(memory_size=10, opts=opts, model_type="vlpythia", num_hidden_layers=3, distillation_layer_weighing_strategy="discounted",
              distillation_layer=None)
    assert FeatureDistillation(**kw).teacher_cache_dtype == torch.float32
    assert FeatureDistillation(teacher_cache_dtype="fp32", **kw).teacher_cache_dtype == torch.float32
    assert FeatureDistillation(teacher_cache_dtype=torch.bfloat16, **kw).teacher_cache_dtype == torch.bfloat16
    with pytest.raises(ValueError):
        FeatureDistillation(teacher_cache_dtype="fp8", **kw)
    with pytest.raises(ValueError):
        FeatureDistillation(teacher_cache_dtype=torch.float16, **kw)
    fd, _, _ = _make()
    with pytest.raises(ValueError):
        fd.build_teacher_cache(dtype="fp8")
    assert fd._tcache is None
