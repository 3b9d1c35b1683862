"""Right padding of the text to a tile multiple (``VLPythiaForCausalLM.text_bucket``): the engine appends masked positions
behind the text so that rows = B * (P + T) tile the fast GEMMs, and trims what callers see.  Appended positions are invisible to every
real query (causal), carry no loss term and leave the rotary positions of real tokens alone, so:

  * fp32, forced padding (text_bucket = 8: T = 6 -> S = 16): the reference goldens hold at their existing 1e-3 -- model, MAFED replay
    step, Trainer sequence.  The golden batches are left-padded, so left and right pads coexist in a sample;
  * fp32, padded == unpadded at caller positions;
  * bf16, the smallest shape that tiles (B = 16, P = 104, T = 23 -> 24, rows = 2048): no GEMM of a padded training step reaches the
    register-staged fallback kernel (``mafed_gemm_fallback_launches``) -- unpadded, they do;
  * the teacher cache stores rows at the padded length and refuses a batch of another length.
"""
import dataclasses
import types

import numpy as np
import pytest
import torch

from oracle import vlpythia_ref as R
from tests.helpers import G3_VARIANTS, TINY, g3_spec, golden_setup, load_golden, tiny_cfg
from tests.test_gpu_model import TOL, check_named_grads, close, grad_norms, make_fd_spec, to_dev
from tests.test_gpu_replay import _conf

pytestmark = pytest.mark.gpu
DEV = "cuda"


def build_model(cfg, sd, dtype=torch.float32, text_bucket=None):
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    mc = VLPythiaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        vision_hidden_size=cfg.vision_hidden_size, num_vision_tokens=cfg.num_vision_tokens)
    m = VLPythiaForCausalLM(mc, compute_dtype=dtype, device=DEV, text_bucket=text_bucket)
    m.load_state_dict(sd, strict=True)
    return m


# ---- the pad launch itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,Tp", [(3, 7, 8), (16, 23, 24), (5, 6, 6), (300, 23, 39)])
@pytest.mark.parametrize("with_labels", [True, False])
def test_pad_text_batch_kernel(B, T, Tp, with_labels):
    from mafed_amd import ops
    g = torch.Generator().manual_seed(B * 100 + T)
    ids = torch.randint(1, 1 << 40, (B, T), generator=g).to(DEV)
    am = torch.randint(0, 2, (B, T), generator=g).to(DEV)
    lab = torch.randint(-100, 1000, (B, T), generator=g).to(DEV) if with_labels else None
    pi, pm, pl = ops.pad_text_batch(ids, am, lab, Tp)
    assert pi.shape == pm.shape == (B, Tp) and pi.dtype == pm.dtype == torch.int64 and pi.is_contiguous() and pm.is_contiguous()
    assert torch.equal(pi[:, :T], ids) and torch.equal(pm[:, :T], am)
    assert bool((pi[:, T:] == 0).all()) and bool((pm[:, T:] == 0).all())
    if with_labels:
        assert pl.shape == (B, Tp) and torch.equal(pl[:, :T], lab) and bool((pl[:, T:] == -100).all())
    else:
        assert pl is None


# ---- 1. goldens under forced padding, fp32 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_forward_backward_vs_reference_golden_padded(name):
    """tests/test_gpu_model.py::test_forward_backward_vs_reference_golden with text_bucket = 8 (t64 / t128 / t256: S = 14 -> 16; m64's
    S = 64 is a multiple already and runs as it is)."""
    cfg, sd, tsd, batch, g = golden_setup(name)
    model = build_model(cfg, sd, text_bucket=8)
    B, T = batch["input_ids"].shape
    P = cfg.num_vision_tokens
    assert model.padded_text_len(B, T) == T + (-(P + T)) % 8
    assert name == "m64" or model.padded_text_len(B, T) > T
    assert bool((batch["attention_mask"][:, 0] == 0).any()), "the golden batch is left-padded: both pads in one sample"
    out = model(**to_dev(batch), output_hidden_states=True, return_dict=True)
    assert out.logits.shape == (B, T, cfg.vocab_size) and out.logits.is_contiguous()
    close(out.loss, float(g["g1/loss"]), TOL, "loss")
    close(out.logits, g["g1/logits_text"], TOL, "logits (text positions)")
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1
    for i, hs in enumerate(out.hidden_states):
        assert hs.shape == (B, P + T, cfg.hidden_size) and hs.is_contiguous()
        close(hs, g[f"g1/hidden/{i}"], TOL, f"hidden {i}")
    model.zero_grad()
    out.loss.backward()
    names, norms = grad_norms(model, cfg)
    close(norms, g["g2/grad_norms"], TOL, "per-parameter grad norms")
    close(float(np.sqrt((norms ** 2).sum())), float(g["g2/grad_norm_total"]), TOL, "global grad norm")
    check_named_grads(model, g, "g2/", TOL)
    with torch.no_grad():   # the evaluation forward pads and trims as well
        ev = model(**to_dev(batch), output_hidden_states=True, return_dict=True)
    assert ev.logits.shape == (B, T, cfg.vocab_size) and ev.logits.is_contiguous()
    close(ev.loss, float(g["g1/loss"]), TOL, "loss (no_grad)")
    close(ev.logits, g["g1/logits_text"], TOL, "logits (no_grad)")
    close(ev.hidden_states[-1], g[f"g1/hidden/{cfg.num_hidden_layers}"], TOL, "last hidden (no_grad)")


# ---- 2. MAFED replay under forced padding, fp32 --------------------------------------------------------------------------------------
def _oracle_replay(cfg, sd, tsd, batch, spec):
    """The oracle's replay step in float64: (loss, {name: gradient})."""
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    tp = {k: v.double() for k, v in tsd.items()}
    b64 = dict(batch)
    b64["patch_embeddings"] = batch["patch_embeddings"].double()
    loss, _, _ = R.mafed_replay_loss(params, tp, b64, cfg, spec, task_id=1)
    loss.backward()
    return float(loss.detach()), {k: (p.grad if p.grad is not None else torch.zeros_like(p.detach())) for k, p in params.items()}


REPLAY_CASES = [  # (loss, modality weights) -> golden variant, or None: no golden of that pair, the oracle itself at the same bound
    ("mse", "equal", "equal_discounted_g09_mse"), ("mse", "balanced", "balanced_discounted_g05_mse"),
    ("cosine", "equal", None), ("cosine", "balanced", "balanced_discounted_g05_cosine"),
    ("cls+cosine", "equal", None), ("cls+cosine", "balanced", "cls_cosine"),
]


@pytest.mark.parametrize("loss_kind,modality,vname", REPLAY_CASES)
def test_mafed_replay_vs_reference_golden_padded(loss_kind, modality, vname):
    """tests/test_gpu_model.py::test_mafed_replay_vs_reference_golden on config t64 with text_bucket = 8 on student and teacher: the mask
    sums, the LayerNorm-backward injection (mse, cosine), the trimmed generic path (CLS) and the dict side effects.  The goldens hold
    balanced weights for all three losses and equal weights for mse; equal x {cosine, cls+cosine} is checked against the float64 oracle
    that generated the goldens, at the same bound."""
    cfg, sd, tsd, batch, g = golden_setup("t64")
    B, T = batch["input_ids"].shape
    P = cfg.num_vision_tokens
    if vname is not None:
        spec = g3_spec(vname, cfg, g)
    else:
        base = g3_spec("cls_cosine" if loss_kind == "cls+cosine" else "balanced_discounted_g05_cosine", cfg, g)
        spec = dataclasses.replace(base, modality=modality)
    assert spec.modality == modality and spec.cls == (loss_kind == "cls+cosine") and (spec.loss == "cosine") == (loss_kind != "mse")
    model, teacher = build_model(cfg, sd, text_bucket=8), build_model(cfg, tsd, text_bucket=8)
    assert model.padded_text_len(B, T) == T + 2
    fd, spec = make_fd_spec(cfg, spec, teacher, B)
    assert fd.past_model.text_bucket == 8
    mem = to_dev(batch)
    fd.mem_dataloader = [mem]
    model.zero_grad()
    loss, n_ex = fd.replay(model)
    assert n_ex == B and "labels" not in mem
    assert mem["input_ids"].shape == (B, T) and mem["attention_mask"].shape == (B, T), "the caller's batch keeps its shapes"
    if not spec.cls:
        assert mem["lang_masks"].shape == (B, P + T) and mem["image_masks"].shape == (B, P + T)
        assert torch.equal(mem["lang_masks"][:, P:], mem["attention_mask"]) and int(mem["lang_masks"][:, :P].sum()) == 0
    loss.backward()
    if vname is not None:
        pre = f"g3/{vname}/"
        close(loss, float(g[pre + "loss"]), TOL, "replay loss")
        if not spec.cls:
            close(fd.last_modality_losses.reshape(-1), g[pre + "per_call_losses"], TOL, "per-layer lang/vision losses")
        names, norms = grad_norms(model, cfg)
        close(norms, g[pre + "grad_norms"], TOL, "grad norms")
        close(float(np.sqrt((norms ** 2).sum())), float(g[pre + "grad_norm_total"]), TOL, "global grad norm")
        check_named_grads(model, g, pre, TOL)
    else:
        o_loss, o_grads = _oracle_replay(cfg, sd, tsd, batch, spec)
        close(loss, o_loss, TOL, "replay loss (oracle)")
        for k, og in o_grads.items():
            close(model._g(k), og, TOL, f"grad {k} (oracle)")


# ---- 3. padded equals unpadded, fp32 -------------------------------------------------------------------------------------------------
def test_padded_equals_unpadded_fp32():
    """Tiny config, B = 3, T = 7, P = 8 (S = 15 -> 16), left-padded samples.  Measured on gfx950: hidden states and logits differ by
    exactly zero -- the fp32 kernels sum every output element in an order that does not depend on the row count -- so equality is
    asserted; gradients at the golden bound; row 0 of the embedding gradient (the pad id; no sample uses id 0 as a real token)
    identical."""
    cfg = tiny_cfg("t64")
    sd = R.init_weights(cfg, seed=11, bias_std=0.02, ln_jitter=0.05)
    batch = R.make_batch(cfg, 3, 7, seed=12, pad=True, n_answer=3)
    assert cfg.num_vision_tokens == 8
    assert bool((batch["input_ids"][batch["attention_mask"] == 1] != 0).all())
    runs = {}
    for tb in (0, 8):
        m = build_model(cfg, sd, text_bucket=tb)
        assert m.padded_text_len(3, 7) == (8 if tb else 7)
        out = m(**to_dev(batch), output_hidden_states=True, return_dict=True)
        m.zero_grad()
        out.loss.backward()
        torch.cuda.synchronize()
        runs[tb] = (out, m)
    (a, ma), (b, mb) = runs[0], runs[8]
    worst = 0.0
    for what, x, y in [("logits", a.logits, b.logits)] + [(f"hidden {i}", x, y) for i, (x, y) in enumerate(zip(a.hidden_states, b.hidden_states))]:
        assert x.shape == y.shape, what
        rel = float((x.detach().double() - y.detach().double()).abs().max() / x.detach().double().abs().max())
        print(f"[pad] {what}: max rel diff {rel:.3e}")
        worst = max(worst, rel)
        assert rel <= 1e-6, (what, rel)
        assert torch.equal(x, y), what
    assert float(a.loss.detach()) == float(b.loss.detach())
    for name in ma._params_by_name:
        close(mb._g(name), ma._g(name), TOL, f"grad {name}")
    ea, eb = ma._g("gpt_neox.embed_in.weight"), mb._g("gpt_neox.embed_in.weight")
    assert torch.equal(ea[0], eb[0]), "the appended positions (id 0) added something to the pad id's embedding gradient"


# ---- 4. bf16, the smallest shape that tiles ------------------------------------------------------------------------------------------
BF = dict(h=256, L=2, H=4, P=104, B=16, V=512, Dv=128)   # (Dv: the projector's weight gradient is an [h, Dv] product, N % 128)


def _bf_cfg():
    t = BF
    return R.RefConfig(vocab_size=t["V"], hidden_size=t["h"], num_hidden_layers=t["L"], num_attention_heads=t["H"],
                       intermediate_size=4 * t["h"], vision_hidden_size=t["Dv"], num_vision_tokens=t["P"])


_bf_shared = {}


def _bf_setup(T):
    """(cfg, student weights, teacher weights, batch) at text length T, built once per T and left unchanged."""
    if T not in _bf_shared:
        cfg = _bf_cfg()
        sd = R.init_weights(cfg, seed=21, bias_std=0.02, ln_jitter=0.05)
        tsd = R.perturb(sd, seed=22, std=5e-3)
        _bf_shared[T] = (cfg, sd, tsd, R.make_batch(cfg, BF["B"], T, seed=23 + T, pad=True, n_answer=3))
    return _bf_shared[T]


def _fd(cfg, teacher, B):
    spec = R.DistillSpec(distillation_coeff=1.0, replay_coeff=1.0, modality="balanced", layer_strategy="discounted", gamma=0.5)
    return make_fd_spec(cfg, spec, teacher, B)[0]


def _replay_once(cfg, sd, tsd, batch, dtype, text_bucket):
    from mafed_amd import ops
    student, teacher = build_model(cfg, sd, dtype, text_bucket), build_model(cfg, tsd, dtype, text_bucket)
    fd = _fd(cfg, teacher, BF["B"])
    fd.mem_dataloader = [to_dev(batch)]
    student.zero_grad()
    torch.cuda.synchronize()
    n0 = ops.gemm_fallback_launches()
    loss, _ = fd.replay(student)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=float(loss.detach()), gn=float(student.flat_grads.double().norm()), mod=fd.last_modality_losses.float().cpu().numpy(),
                fallback=ops.gemm_fallback_launches() - n0)


def test_bf16_padded_step_tracks_the_fp32_engine():
    """T = 23 (auto: T' = 24, rows = 16 * 128 = 2048) in bf16 against the exact fp32 kernels on the same batch, unpadded: loss, per-layer
    language / vision losses and the gradient norm within 2e-2, the bf16 bound of tests/test_gpu_oracle_fullshape.py."""
    cfg, sd, tsd, batch = _bf_setup(23)
    ref = _replay_once(cfg, sd, tsd, batch, torch.float32, 0)
    got = _replay_once(cfg, sd, tsd, batch, torch.bfloat16, None)
    print(f"[pad] bf16 padded vs fp32: loss {got['loss']:.6f} / {ref['loss']:.6f}, grad norm {got['gn']:.5f} / {ref['gn']:.5f}")
    assert ref["fallback"] == 0, "the fp32 engine launches no bf16 GEMM"
    assert abs(got["loss"] - ref["loss"]) <= 2e-2 * abs(ref["loss"]), (got["loss"], ref["loss"])
    rel = np.abs(got["mod"] - ref["mod"]) / np.maximum(np.abs(ref["mod"]), 1e-12)
    assert float(rel.max()) <= 2e-2, (rel, got["mod"], ref["mod"])
    assert abs(got["gn"] - ref["gn"]) <= 2e-2 * ref["gn"], (got["gn"], ref["gn"])


def _trainer_step(T, text_bucket, incremental_norm=True, fused=True):
    from mafed_amd import Trainer, ops
    cfg, sd, tsd, batch = _bf_setup(T)
    student, teacher = build_model(cfg, sd, torch.bfloat16, text_bucket), build_model(cfg, tsd, torch.bfloat16, text_bucket)
    fd = _fd(cfg, teacher, BF["B"])
    tr = Trainer(student, fd, _conf(lr=1e-4), task_id=1, incremental_norm=incremental_norm)
    tr.fused_norm_squares = fused
    recs = []
    torch.cuda.synchronize()
    n0 = ops.gemm_fallback_launches()
    for i in range(2):   # a replay step (student + teacher + distillation) each; the task batch is dropped on replay steps
        fd.mem_dataloader = [to_dev(batch)]
        recs.append(tr.step(to_dev(batch), i))
    tr.join()
    torch.cuda.synchronize()
    assert all(r["branch"] == "replay" and r["stepped"] for r in recs)
    return ops.gemm_fallback_launches() - n0, [float(r["grad_norm"]) for r in recs], [float(r["loss"]) for r in recs]


def test_padded_training_step_stays_off_the_fallback_gemm():
    """Trainer.step (MAFED replay: student, teacher, backward, clip, AdamW) in bf16 at B = 16, P = 104.  T = 23 with the default
    ``text_bucket="auto"`` runs at T' = 24: no launch reaches the register-staged kernel, exactly as at T = 24.  With text_bucket = 0
    rows = 2032 (2032 % 64 = 48) and every product of the step falls through to it."""
    n_auto, _, loss_auto = _trainer_step(23, None)
    n_aligned, _, _ = _trainer_step(24, None)
    n_off, _, loss_off = _trainer_step(23, 0)
    print(f"[pad] fallback launches in two steps: T=23 auto {n_auto}, T=24 {n_aligned}, T=23 off {n_off}")
    assert n_aligned == 0, "the aligned shape itself reaches the fallback kernel: the test's shape is wrong"
    assert n_auto == 0, f"{n_auto} GEMM launches of the padded step reached the register-staged kernel"
    assert n_off > 0, "text_bucket = 0 must leave the ragged route as it was"
    assert abs(loss_auto[0] - loss_off[0]) <= 2e-2 * abs(loss_off[0]), (loss_auto, loss_off)   # the same step, two kernel routes (bf16)


def test_padded_step_clip_norm_fused_squares_vs_one_pass():
    """The clip norm of the padded T = 23 step from the backward's partials (matrix squares from the weight-gradient launches, ranges from
    the hooks) equals the one-pass ``gradnorm_clip`` within 2e-3, the bound of tests/test_gpu_overwrite.py (run-to-run noise of a bf16
    backward's atomics).  Whether the squares ride in the GEMM epilogue is the library's answer per row count: at the 410M width the
    padded row count 16 * 280 gets it, the ragged 16 * 279 does not."""
    from mafed_amd import ops
    _, fused, _ = _trainer_step(23, None, incremental_norm=True, fused=True)
    _, onepass, _ = _trainer_step(23, None, incremental_norm=False, fused=False)
    print(f"[pad] clip norms fused {fused} one-pass {onepass}")
    assert abs(fused[0] - onepass[0]) <= 2e-3 * onepass[0], (fused, onepass)
    assert abs(fused[1] - onepass[1]) <= 2e-3 * onepass[1], (fused, onepass)
    layer = lambda h, rows: [(3 * h, h, rows), (h, h, rows), (4 * h, h, rows), (h, 4 * h, rows)]
    assert ops.gemm_grouped_fuses_sumsq(layer(1024, 16 * 280) * 2, True, False)
    assert not ops.gemm_grouped_fuses_sumsq(layer(1024, 16 * 279) * 2, True, False)


# ---- 6. Trainer sequence under forced padding ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [False, True])
def test_trainer_sequence_vs_reference_golden_padded(pipeline):
    """tests/test_gpu_model.py::test_trainer_sequence_vs_reference_golden with text_bucket = 8: task steps, MAFED replay steps,
    accumulation, clip, AdamW, schedule -- loss, grad-norm and lr against the golden sequence at its bounds."""
    from mafed_amd import FeatureDistillation, Trainer
    g = load_golden("trainer_t64.npz")
    name, seed = "t64", int(g["meta/seed"])
    cfg, t = tiny_cfg(name), TINY[name]
    sd = R.init_weights(cfg, seed=seed, bias_std=0.02, ln_jitter=0.05)
    tsd = R.perturb(sd, seed=seed + 100, std=5e-3)
    model, teacher = build_model(cfg, sd, text_bucket=8), build_model(cfg, tsd, text_bucket=8)
    assert model.padded_text_len(t["B"], t["T"]) > t["T"]
    opts = types.SimpleNamespace(tasks=["a", "b", "c"], batch_size=t["B"], seed=42, pin_mem=False, accumulate_grad_batches=4)
    fd = FeatureDistillation(memory_size=100, opts=opts, model_type="vlpythia", num_hidden_layers=cfg.num_hidden_layers - 1,
                             distillation_modality_weighing_strategy="balanced", distillation_layer_weighing_strategy="discounted",
                             gamma=0.5, distillation_layer=None, distillation_coeff=1.0, replay_coeff=1.0)
    fd._update_model(teacher)
    fd.task_id = 1
    fd.num_vision_tokens = cfg.num_vision_tokens
    conf = types.SimpleNamespace(accumulate_grad_batches=4, replay_interval=4, grad_norm=2.0, learning_rate=float(g["meta/lr"]),
                                 betas=(0.9, 0.98), weight_decay=0.01, optim="adamw", warmup_steps=int(g["meta/warmup"]),
                                 total_steps=int(g["meta/total_steps"]))
    tr = Trainer(model, fd, conf, task_id=1, pipeline_optimizer=pipeline)
    branches, losses, gns, lrs, sums = [], [], [], [], []
    for bi in range(8):
        batch = R.make_batch(cfg, t["B"], t["T"], seed=seed + 10 + bi, pad=True, n_answer=3)
        mem = R.make_batch(cfg, t["B"], t["T"], seed=seed + 50 + bi, pad=True, n_answer=3)
        fd.mem_dataloader = [to_dev(mem)]
        rec = tr.step(to_dev(batch), bi)
        branches.append(int(rec["branch"] == "replay"))
        losses.append(float(rec["loss"]))
        if rec["stepped"]:
            gns.append(float(rec["grad_norm"]))
            lrs.append(rec["lr"])
            tr.join()
            sums.append(float(sum(p.detach().double().sum() for p in model.parameters())))
    assert branches == list(g["seq/branch"].astype(int))
    close(np.array(losses), g["seq/loss"], TOL, "loss sequence")
    close(np.array(gns), g["seq/grad_norm"], TOL, "grad-norm sequence")
    close(np.array(lrs), g["seq/lr"], 1e-9, "lr sequence")
    close(np.array(sums), g["seq/checksum"], 1e-5, "parameter checksum after each optimiser step")


# ---- 7. teacher cache ----------------------------------------------------------------------------------------------------------------
def test_teacher_cache_is_stored_at_the_padded_length_and_refuses_another():
    """fp32 compute with text_bucket = "auto" at B = 16, P = 104: a memory of T = 23 samples is cached at S = 104 + 24 = 128; steps fed
    from the cache equal the steps that run the teacher forward bit for bit (first step: same weights, same batch, same teacher bits),
    as tests/test_gpu_replay.py requires of the unpadded cache.  A T = 27 batch (T' = 32, S = 136) against that cache raises."""
    from mafed_amd import Trainer
    from mafed_amd.methods import HBMReplayBuffer
    cfg = _bf_cfg()
    B, P = BF["B"], BF["P"]
    sd = R.init_weights(cfg, seed=31, bias_std=0.02, ln_jitter=0.05)
    tsd = R.perturb(sd, seed=32, std=5e-3)
    data = R.make_batch(cfg, 2 * B + 3, 23, seed=33, pad=True, n_answer=3)
    data["patch_embeddings"] = data["patch_embeddings"].to(torch.bfloat16).float()   # the buffer stores bf16 features
    longer = R.make_batch(cfg, 2 * B + 3, 27, seed=34, pad=True, n_answer=3)

    def run(cached):
        model, teacher = build_model(cfg, sd, torch.float32, "auto"), build_model(cfg, tsd, torch.float32, "auto")
        fd = _fd(cfg, teacher, B)
        mem = HBMReplayBuffer(B, DEV, seed=9)
        mem.add(data)
        fd.mem_dataloader = mem
        calls = []
        if cached:
            fd.build_teacher_cache()
            assert fd._tcache["S"] == P + 24 and fd._tcache["states"].shape[2] == P + 24
            orig = fd.past_model.hidden_states_upto
            fd.past_model.hidden_states_upto = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        tr = Trainer(model, fd, _conf(lr=1e-3), task_id=1, pipeline_optimizer=True)
        task = {k: v[:B].to(DEV) for k, v in data.items()}
        losses, gns = [], []
        for i in range(2):     # T = 23, then T = 23 again
            rec = tr.step(task, i)
            losses.append(rec["loss"]); gns.append(rec["grad_norm"])
        tr.join()
        torch.cuda.synchronize()
        assert not calls, "the teacher forward ran although its states are cached"
        out = ([float(x) for x in losses], [float(x) for x in gns])
        if cached:
            for k in ("input_ids", "attention_mask", "labels"):
                mem.data[k] = longer[k].to(DEV)
            mem._next = None
            with pytest.raises(RuntimeError, match="teacher cache"):
                fd.replay(model)
            torch.cuda.synchronize()
        return out

    la, ga = run(False)
    lb, gb = run(True)
    assert la[0] == lb[0] and ga[0] == gb[0], (la, lb, ga, gb)
    assert all(abs(a - b) <= 1e-6 * abs(a) for a, b in zip(la, lb)) and all(abs(a - b) <= 1e-5 * abs(a) for a, b in zip(ga, gb)), (la, lb, ga, gb)
    assert la[0] != la[1]
