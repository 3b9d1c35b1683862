"""Shared helpers for the parity tests (test infrastructure; may import oracle/)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vlpythia_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TINY = {
    "t64": dict(h=128, H=2, L=3, V=512, P=8, T=6, B=3, Dv=32),
    "t128": dict(h=256, H=2, L=2, V=256, P=8, T=6, B=2, Dv=32),
    "t256": dict(h=256, H=1, L=2, V=256, P=8, T=6, B=2, Dv=32),
    "m64": dict(h=128, H=2, L=4, V=600, P=40, T=24, B=3, Dv=48),
}


def tiny_cfg(name):
    t = TINY[name]
    return R.RefConfig(vocab_size=t["V"], hidden_size=t["h"], num_hidden_layers=t["L"], num_attention_heads=t["H"],
                       intermediate_size=4 * t["h"], vision_hidden_size=t["Dv"], num_vision_tokens=t["P"])


def load_golden(fname):
    return np.load(os.path.join(GOLDEN, fname), allow_pickle=False)


def golden_setup(name):
    """(cfg, student weights, teacher weights, batch, golden) exactly as oracle/gen_golden.py built them."""
    g = load_golden(f"model_{name}.npz")
    cfg = tiny_cfg(name)
    seed = int(g["meta/seed"])
    sd = R.init_weights(cfg, seed=seed, bias_std=0.02, ln_jitter=0.05)
    chk = float(sum(v.double().abs().sum() for v in sd.values()))
    assert abs(chk - float(g["meta/weight_checksum"])) < 1e-6 * chk, "deterministic weight generator drifted"
    tsd = R.perturb(sd, seed=seed + 100, std=5e-3)
    batch = {k: torch.from_numpy(g["batch/" + k]) for k in ("input_ids", "attention_mask", "labels", "patch_embeddings")}
    return cfg, sd, tsd, batch, g


G3_VARIANTS = {
    "balanced_discounted_g05_mse": dict(modality="balanced", layer_strategy="discounted", gamma=0.5),
    "equal_discounted_g09_mse": dict(modality="equal", layer_strategy="discounted", gamma=0.9),
    "equal_equal_mse": dict(modality="equal", layer_strategy="equal"),
    "balanced_single_mse": dict(modality="balanced", layer_strategy="single", distillation_layer="min1"),
    "balanced_discounted_g05_cosine": dict(modality="balanced", layer_strategy="discounted", gamma=0.5, loss="cosine"),
    "cls_cosine": dict(modality="balanced", layer_strategy="discounted", gamma=0.5, loss="cosine", cls=True),
    "adaptive_discounted_g05_mse": dict(modality="adaptive", layer_strategy="discounted", gamma=0.5),
    "balanced_cumulative_mse": dict(modality="balanced", layer_strategy="cumulative", distillation_layer="nh-1", gamma=0.8),
}


def g3_spec(vname, cfg, g):
    kw = dict(G3_VARIANTS[vname])
    nh = cfg.num_hidden_layers - 1
    if kw.get("distillation_layer") == "min1":
        kw["distillation_layer"] = min(1, nh - 1)
    elif kw.get("distillation_layer") == "nh-1":
        kw["distillation_layer"] = nh - 1
    if kw["modality"] == "adaptive":
        kw["lang_coeff"] = torch.from_numpy(g["g3/adaptive_lang_coeff"])
    return R.DistillSpec(distillation_coeff=1.5, replay_coeff=0.7, **kw)


def ewc_setup(name="t64"):
    """Inputs of oracle/gen_golden.py::gen_ewc_fixture: (cfg, golden, anchor weights sd0, task-1 weights sd1, the two importance
    loaders, the step batch, the synthetic Fisher diagonal)."""
    g = load_golden(f"ewc_{name}.npz")
    cfg = tiny_cfg(name)
    t = TINY[name]
    seed = int(g["seed"])
    sd0 = R.init_weights(cfg, seed=seed)
    loaders = [[R.make_batch(cfg, t["B"], t["T"], seed=seed + 10 * r + i, pad=True) for i in range(2)] for r in range(2)]
    sd1 = R.perturb(sd0, seed=seed + 1, std=2e-3)
    batch = R.make_batch(cfg, t["B"], t["T"], seed=seed + 5, pad=True)
    syn = {k: v.abs() for k, v in R.init_weights(cfg, seed=seed + 7).items()}
    return cfg, g, sd0, sd1, loaders, batch, syn


DECODE_CASES = {"t64": "t64", "t64_eos": "t64", "t64_row0": "t64", "m64": "m64", "t128": "t128"}


def decode_setup(case):
    """Inputs of oracle/gen_golden.py::gen_decode_fixture: (cfg, weights, batch, eos or None, max_new, golden tokens, step logits, top-2 gaps)."""
    g = load_golden("decode.npz")
    name = DECODE_CASES[case]
    cfg, t = tiny_cfg(name), TINY[name]
    seed = int(g["seed"])
    sd = R.init_weights(cfg, seed=seed)
    batch = R.make_batch(cfg, t["B"], t["T"], seed=seed + 1, pad=True)
    if case.endswith("_row0"):
        batch = {k: v[:1].clone() for k, v in batch.items()}
    eos = int(g[f"{case}/eos"])
    return (cfg, sd, batch, None if eos < 0 else eos, int(g[f"{case}/max_new"]), torch.from_numpy(g[f"{case}/tokens"]),
            torch.from_numpy(g[f"{case}/step_logits"]), torch.from_numpy(g[f"{case}/top2_gap"]))


CLIP_TINY = {  # mirrors oracle/gen_golden.py::CLIP_TINY
    "c17": dict(hidden=128, heads=2, layers=3, ff=512, image=56, patch=14, B=2, lm=dict(h=128, H=2, L=2, V=384, T=6)),
    "c50": dict(hidden=192, heads=3, layers=4, ff=640, image=98, patch=14, B=3, lm=dict(h=128, H=2, L=2, V=384, T=7)),
}


def clip_setup(name):
    """Inputs of oracle/gen_golden.py::gen_clip_fixture: (tower cfg, tower weights, pixels, LM cfg, LM weights, text batch, golden)."""
    from oracle import clip_vit_ref as C
    g = load_golden(f"clip_{name}.npz")
    t = CLIP_TINY[name]
    seed = int(g["seed"])
    cc = C.ClipVisionRefConfig(hidden_size=t["hidden"], num_hidden_layers=t["layers"], num_attention_heads=t["heads"],
                               intermediate_size=t["ff"], image_size=t["image"], patch_size=t["patch"])
    csd = C.init_weights(cc, seed=seed)
    chk = float(sum(v.double().abs().sum() for v in csd.values()))
    assert abs(chk - float(g["weight_checksum"])) < 1e-6 * chk, "deterministic CLIP weight generator drifted"
    pixels = C.make_pixels(cc, t["B"], seed + 1)
    lm = t["lm"]
    cfg = R.RefConfig(vocab_size=lm["V"], hidden_size=lm["h"], num_hidden_layers=lm["L"], num_attention_heads=lm["H"],
                      intermediate_size=4 * lm["h"], vision_hidden_size=cc.hidden_size, num_vision_tokens=cc.num_patches)
    sd = R.init_weights(cfg, seed=seed + 2, bias_std=0.02, ln_jitter=0.05)
    batch = R.make_batch(cfg, t["B"], lm["T"], seed=seed + 3, pad=True, n_answer=3)
    return cc, csd, pixels, cfg, sd, batch, g


# ---------------------------------------------------------------------------------------------------------------
# scale-aware comparison and the fp64 distillation-only oracle (MAFED feature-distillation parity)
# ---------------------------------------------------------------------------------------------------------------
def _f64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().double().numpy()
    return np.asarray(x, np.float64)


def rel_err(a, ref, scale=None):
    """max|a - ref| / S with S = max|ref| (or max|scale| when given: a cancellation residue such as the column sum of a
    weight gradient is judged against the tensor it was summed from).  A zero reference scale gives 0 when ``a`` is exactly
    zero as well and inf otherwise."""
    a, ref = _f64(a), _f64(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if not a.size:
        return 0.0
    s = float(np.abs(_f64(ref if scale is None else scale)).max())
    err = float(np.abs(a - ref).max())
    if s == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / s


def assert_rel_close(a, ref, rtol, what="", scale=None, atol0=0.0):
    """err <= rtol * max|ref| (per tensor; ``scale`` as in rel_err).  A reference that is exactly zero must come out within
    ``atol0`` (default: exactly zero).  Returns the measured relative error."""
    a64, ref64 = _f64(a), _f64(ref)
    assert a64.shape == ref64.shape, (what, a64.shape, ref64.shape)
    s = float(np.abs(_f64(ref if scale is None else scale)).max()) if ref64.size else 0.0
    err = float(np.abs(a64 - ref64).max()) if a64.size else 0.0
    if s == 0.0:
        print(f"[rel] {what}: zero reference, max|got| {err:.3e} (atol {atol0:.1e})")
        assert err <= atol0, f"{what}: reference is exactly zero, got max |{err:.3e}| > {atol0:.1e}"
        return 0.0
    r = err / s
    print(f"[rel] {what}: rel err {r:.3e} (bound {rtol:.1e})")
    assert r <= rtol, f"{what}: max err {err:.3e} = {r:.3e} x max|ref| {s:.3g} > rtol {rtol:.1e}"
    return r


# Bounds of the distillation parity checks (tests/test_gpu_model.py, tests/test_gpu_kernels.py), each measured on an MI355X and
# guarded on the CPU by tests/test_distill_guard.py: a mutated fp64 oracle (distillation_coeff x 1.01, lang/vision weights swapped,
# one layer coefficient dropped, the first valid text token classed as pad) must fail every check it applies to.
# (measured worst case on gfx950 in brackets)
DISTILL_RTOL = 2e-5           # fp32 native distillation-only step vs fp64 oracle: loss, per-layer lang/vision losses, every gradient [3.5e-6]
DISTILL_RTOL_INJECT = 1e-3    # native grad(replay + 10x distillation) - grad(replay only) vs 10x the fp64 distillation-only gradient
#                               [3.5e-3 at 1x: the fp32 rounding of the CE gradient, 1e3 times larger, sets the floor; 10x lifts the term above it]
DISTILL_RTOL_BF16 = 5e-2      # bf16 step at production width vs fp64 oracle (loss and gradients) [1.3e-2]
KERNEL_RTOL = 2e-5            # distill_fwd / distill_bwd / distill_combine vs fp64 [6.2e-6]
LN_INJECT_RTOL = 1e-4         # LayerNorm-backward injection dx(with) - dx(without) vs fp64 [1.1e-5]
GUARD_MARGIN = 3.0            # each mutation must exceed its bound by this factor


def distill_variant_cases():
    """(config, variant) pairs of G3_VARIANTS that distil at least one layer (cumulative needs L >= 3)."""
    return [(n, v) for n in ("t64", "m64", "t128", "t256") for v in G3_VARIANTS
            if not (G3_VARIANTS[v]["layer_strategy"] == "cumulative" and TINY[n]["L"] < 3)]


def distill_only_fp64(cfg, sd, tsd, batch, spec):
    """fp64 oracle of the distillation term alone (replay_coeff = 0): {"loss", "modality" [nl, 2] or None, "grads" {name: tensor}}.
    Parameters that the distillation term does not reach get an exact zero gradient."""
    import dataclasses
    spec = dataclasses.replace(spec, replay_coeff=0.0)
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    tp = {k: v.double() for k, v in tsd.items()}
    b64 = dict(batch)
    b64["patch_embeddings"] = batch["patch_embeddings"].double()
    loss, _, per_layer = R.mafed_replay_loss(params, tp, b64, cfg, spec, task_id=1)
    loss.backward()
    layers = sorted(per_layer)
    modality = None if spec.cls else torch.stack([torch.stack([per_layer[l]["lang"], per_layer[l]["vision"]]) for l in layers]).detach()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p.detach())) for k, p in params.items()}
    return {"loss": float(loss.detach()), "modality": modality, "grads": grads}


def distill_parity_errors(got, ref):
    """{quantity: relative error (rel_err)} of ``got`` (layout of distill_only_fp64) against ``ref``: the loss, each layer's lang
    and vision loss, every parameter gradient tensor."""
    errs = {"loss": rel_err(got["loss"], ref["loss"])}
    if ref["modality"] is not None and got.get("modality") is not None:
        m, rm = _f64(got["modality"]).reshape(-1, 2), _f64(ref["modality"])
        assert m.shape == rm.shape, (m.shape, rm.shape)
        for l in range(rm.shape[0]):
            for j, mod in enumerate(("lang", "vision")):
                errs[f"layer {l} {mod} loss"] = rel_err(m[l, j], rm[l, j])
    for k in ref["grads"]:
        errs[f"grad {k}"] = rel_err(got["grads"][k], ref["grads"][k])
    return errs


def check_distill_parity(got, ref, rtol, what=""):
    """Every quantity of distill_parity_errors within rtol (exact zeros where the reference is exactly zero).  Returns the largest."""
    errs = distill_parity_errors(got, ref)
    worst = max(errs, key=errs.get)
    print(f"[rel] {what}: worst {worst} {errs[worst]:.3e} (bound {rtol:.1e}); loss {errs['loss']:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= rtol}
    assert not bad, f"{what}: relative errors above {rtol:.1e}: " + ", ".join(f"{k} {v:.3e}" for k, v in bad.items())
    return errs[worst]


PROD_DISTILL = dict(h=1024, H=16, L=3, V=512, P=256, T=32, B=4, Dv=64)


def prod_case(seed=77):
    """(cfg, student / teacher weights, batch, spec, fp64 distillation-only oracle) of the production-width distillation check.
    Left padding from make_batch; sample 3 has all of its text padded.  Equal modality weights, discounted layers (gamma 0.9)."""
    t = PROD_DISTILL
    cfg = R.RefConfig(vocab_size=t["V"], hidden_size=t["h"], num_hidden_layers=t["L"], num_attention_heads=t["H"],
                      intermediate_size=4 * t["h"], vision_hidden_size=t["Dv"], num_vision_tokens=t["P"])
    sd = R.init_weights(cfg, seed=seed, bias_std=0.02, ln_jitter=0.05)
    tsd = R.perturb(sd, seed=seed + 1, std=5e-3)
    batch = R.make_batch(cfg, t["B"], t["T"], seed=seed + 2, pad=True, n_answer=3)
    batch["attention_mask"][3] = 0
    batch["input_ids"][3] = 0
    batch["labels"][3] = -100
    spec = R.DistillSpec(distillation_coeff=1.5, replay_coeff=0.0, modality="equal", layer_strategy="discounted", gamma=0.9)
    return dict(cfg=cfg, sd=sd, tsd=tsd, batch=batch, spec=spec, ref=distill_only_fp64(cfg, sd, tsd, batch, spec))


# fp64 restatements of the distillation kernels (tests/test_gpu_kernels.py; mutated by tests/test_distill_guard.py)
def distill_rows_fp64(s, t, attention_mask, P, coef, cosine):
    """mafed_distill_fwd / mafed_distill_bwd in float64 from the oracle's masks: (sums [lang_sum, vision_sum, n_lang, n_vision],
    ds = d(coef[0] * lang_sum + coef[1] * vision_sum) / ds)."""
    B, S, h = s.shape
    lang, img = R.modality_masks(attention_mask, P)
    lang, img = lang.reshape(-1).double(), img.reshape(-1).double()
    a, b = s.reshape(-1, h).double().requires_grad_(True), t.reshape(-1, h).double()
    if cosine:
        d = F.cosine_embedding_loss(a, b, torch.ones(a.shape[0], dtype=torch.float64), reduction="none")
    else:
        d = ((a - b) ** 2).sum(-1) / h
    ls, vs = (d * lang).sum(), (d * img).sum()
    c = [float(x) for x in coef]
    (c[0] * ls + c[1] * vs).backward()
    sums = torch.stack([ls.detach(), vs.detach(), lang.sum(), img.sum()])
    return sums, a.grad.view(B, S, h)


def ln_injection_fp64(x, t, attention_mask, S, P, scales, inj_mul):
    """The distillation gradient the LayerNorm backward adds to dx (mafed_layernorm_bwd, teacher != NULL), float64:
    inj_mul > 0: inj_mul * scale[class] * (x - t); inj_mul < 0: |inj_mul| * scale[class] * d/dx (1 - cos(x, t))."""
    rows, h = x.shape
    lang, img = R.modality_masks(attention_mask, P)
    w = abs(inj_mul) * (float(scales[0]) * lang.reshape(-1).double() + float(scales[1]) * img.reshape(-1).double())
    xd, td = x.double().requires_grad_(True), t.double()
    if inj_mul < 0:
        d = F.cosine_embedding_loss(xd, td, torch.ones(rows, dtype=torch.float64), reduction="none")
    else:
        d = 0.5 * ((xd - td) ** 2).sum(-1)
    (w * d).sum().backward()
    return xd.grad


def distill_combine_fp64(sums, layer_coeff, mode, lang_weight=0.5, lang_vec=None):
    """mafed_distill_combine in float64: (loss, per_layer [nl], modality [nl, 2], inject [nl, 4])."""
    s = sums.double()
    c = layer_coeff.double()
    lang, vis = s[:, 0] / s[:, 2], s[:, 1] / s[:, 3]
    if mode == 0:
        lw = (s[0, 2] / (s[0, 2] + s[0, 3])).expand_as(lang)
    elif mode == 1:
        lw = torch.full_like(lang, float(lang_weight))
    else:
        lw = lang_vec.double()
    vw = 1.0 - lw
    per_layer = lw * lang + vw * vis
    inject = torch.stack([c * lw / s[:, 2], c * vw / s[:, 3], torch.zeros_like(c), torch.zeros_like(c)], dim=1)
    return (c * per_layer).sum(), per_layer, torch.stack([lang, vis], dim=1), inject


# ---------------------------------------------------------------------------------------------------------------
# fp64 oracle of the whole training step and of the optimiser sequence (cross-entropy path, backward sweep, AdamW)
# ---------------------------------------------------------------------------------------------------------------
# Bounds of the whole-step parity checks (tests/test_gpu_model.py), each the worst native-against-float64 relative error per tensor
# over all of its cases, measured on an MI355X, times 3 to 10, and guarded on the CPU by tests/test_step_guard.py: a mutated fp64
# oracle (tanh GELU, rotary base 10500, LayerNorm eps 1e-6, key padding ignored, one label dropped, rotary_pct 0.5; for the updates
# AdamW eps 1e-8, beta2 0.999, clip at 2.2, weight decay 0.02) must fail the same comparator by GUARD_MARGIN times the bound.
# (measured worst case on gfx950 in brackets)
STEP_RTOL = 1e-5              # fp32 native forward + backward vs fp64 oracle: loss, text logits, hidden states, every gradient
#                               [1.7e-6: ev, grad layers.0.mlp.dense_h_to_4h.bias; guard ceiling 4.4e-5: rotary base 10500 on t64 and ev]
STEP_RTOL_BF16 = 5e-2         # bf16 step vs fp64 oracle: loss, hidden states, every gradient
#                               [1.2e-2: t256, grad final_layer_norm.weight; guard ceiling 8.4e-2: key padding ignored on m64]
UPDATE_RTOL = 1e-3            # fp32 Trainer, 8 optimiser steps, vs fp64 RefTrainer: final - initial per parameter tensor
#                               [2.4e-4: embed_in.weight, rows of rare tokens; next 7.6e-5; guard ceiling 4.7e-3: weight decay 0.02]

STEP_EDGE = {
    # S = 83 crosses the 64-row attention tile and is no multiple of 16; sample 2 has no label at all (0 / clamp(0, 1e-13))
    "e83": dict(h=128, H=2, L=2, V=384, P=70, T=13, B=3, Dv=48, seed=83),
    # head size 128; V a multiple of 4 and of nothing larger that matters
    "e128": dict(h=256, H=2, L=2, V=260, P=40, T=24, B=2, Dv=32, seed=128),
    # three trips of the CE kernels' 1024-column loop with a short last one: the online log-sum-exp rescale
    "ev": dict(h=128, H=2, L=2, V=2052, P=8, T=6, B=2, Dv=32, seed=2052),
}
STEP_CASES = list(TINY) + list(STEP_EDGE)


def step_case(name):
    """(cfg, weights, batch) of a whole-step parity case: the golden inputs of a TINY config, or a STEP_EDGE config built from the
    oracle's deterministic generators (left padding from make_batch)."""
    if name in TINY:
        cfg, sd, _, batch, _ = golden_setup(name)
        return cfg, sd, batch
    t = STEP_EDGE[name]
    cfg = R.RefConfig(vocab_size=t["V"], hidden_size=t["h"], num_hidden_layers=t["L"], num_attention_heads=t["H"],
                      intermediate_size=4 * t["h"], vision_hidden_size=t["Dv"], num_vision_tokens=t["P"])
    sd = R.init_weights(cfg, seed=t["seed"], bias_std=0.02, ln_jitter=0.05)
    batch = R.make_batch(cfg, t["B"], t["T"], seed=t["seed"] + 1, pad=True, n_answer=3)
    if name == "e83":
        batch["labels"][2] = -100
    return cfg, sd, batch


def step_fp64(cfg, sd, batch):
    """fp64 oracle of one forward + backward: {"loss", "logits" [B, T, V] (text positions), "hidden" (all L + 1), "grads" {name:
    tensor}, "num_heads" (layout of the fused biases)}.  A parameter that the loss does not reach gets exact zeros.  (The oracle keeps the reference's fp32 softmax and
    cross-entropy, and fp32 rotary tables: its own floor is near 1e-7.)"""
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    b64 = dict(batch)
    b64["patch_embeddings"] = batch["patch_embeddings"].double()
    out = R.forward(params, b64, cfg)
    out.loss.backward()
    T = batch["input_ids"].shape[1]
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p.detach())) for k, p in params.items()}
    return {"loss": float(out.loss.detach()), "logits": out.logits[:, -T:].detach().clone(),
            "hidden": [x.detach().clone() for x in out.hidden_states], "grads": grads, "num_heads": cfg.num_attention_heads}


_STEP_REF = {}


def step_ref(name):
    """step_fp64 of step_case(name), computed once and shared (read only)."""
    if name not in _STEP_REF:
        _STEP_REF[name] = step_fp64(*step_case(name))
    return _STEP_REF[name]


def key_bias_mask(n, num_heads):
    """The K third of a fused query_key_value bias [3 h] (rows interleaved per head as [H, {q, k, v}, D]) as a boolean mask."""
    m = np.zeros((num_heads, 3, n // (3 * num_heads)), bool)
    m[:, 1] = True
    return m.reshape(-1)


def step_parity_errors(got, ref, grad_mul=1.0):
    """{quantity: relative error (rel_err)} of ``got`` (layout of step_fp64; "logits" may be absent) against ``ref``: the loss, the
    text logits, every hidden state and every parameter gradient tensor against ``grad_mul`` times the reference's.  The key third
    of a query_key_value bias gradient is mathematically zero (softmax does not see a shift of its row) and rounding noise near 1e-8
    in any implementation: it is judged against the scale of the whole bias gradient, the rest of the bias against its own."""
    errs = {"loss": rel_err(got["loss"], ref["loss"])}
    if "logits" in got:
        errs["logits"] = rel_err(got["logits"], ref["logits"])
    assert len(got["hidden"]) == len(ref["hidden"]), (len(got["hidden"]), len(ref["hidden"]))
    for i, (a, b) in enumerate(zip(got["hidden"], ref["hidden"])):
        errs[f"hidden {i}"] = rel_err(a, b)
    assert set(got["grads"]) == set(ref["grads"])
    for k, r in ref["grads"].items():
        a, r = _f64(got["grads"][k]), grad_mul * _f64(r)
        if k.endswith("query_key_value.bias"):
            km = key_bias_mask(r.size, ref["num_heads"])
            errs[f"grad {k} [q, v]"] = rel_err(a[~km], r[~km])
            errs[f"grad {k} [k]"] = rel_err(a[km], r[km], scale=r)
        else:
            errs[f"grad {k}"] = rel_err(a, r)
    return errs


def check_step_parity(got, ref, rtol, what="", grad_mul=1.0):
    """Every quantity of step_parity_errors within rtol (exact zeros where the reference is exactly zero); the failure names each
    quantity above the bound.  Returns the largest."""
    errs = step_parity_errors(got, ref, grad_mul)
    worst = max(errs, key=errs.get)
    print(f"[rel] {what}: worst {worst} {errs[worst]:.3e} (bound {rtol:.1e}); loss {errs['loss']:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= rtol}
    assert not bad, f"{what}: relative errors above {rtol:.1e}: " + ", ".join(f"{k} {v:.3e}" for k, v in bad.items())
    return errs[worst]


# the optimiser-sequence case: t64, task 1, 16 micro-batches = 8 optimiser steps, the first at lr 0 (warm-up 1)
TRAINER_CASE = dict(name="t64", seed=23, n_batches=16, accumulate=2, replay_interval=4, warmup=1, total_steps=20, lr=1e-3,
                    betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01, grad_clip=2.0, gamma=0.5)


def trainer_case():
    """(cfg, student weights, teacher weights, [(batch, memory batch)] per micro-batch) of TRAINER_CASE."""
    c = TRAINER_CASE
    cfg, t = tiny_cfg(c["name"]), TINY[c["name"]]
    sd = R.init_weights(cfg, seed=c["seed"], bias_std=0.02, ln_jitter=0.05)
    tsd = R.perturb(sd, seed=c["seed"] + 100, std=5e-3)
    batches = [(R.make_batch(cfg, t["B"], t["T"], seed=c["seed"] + 10 + i, pad=True, n_answer=3),
                R.make_batch(cfg, t["B"], t["T"], seed=c["seed"] + 50 + i, pad=True, n_answer=3)) for i in range(c["n_batches"])]
    return cfg, sd, tsd, batches


def trainer_fp64(**overrides):
    """TRAINER_CASE through the oracle's RefTrainer in float64 (MAFED balanced / discounted, both coefficients 1): {"loss" per
    micro-batch, "grad_norm", "lr" per optimiser step, "update" {name: final - initial}}.  ``overrides`` replace RefTrainer fields
    (the guard's mutations)."""
    c = TRAINER_CASE
    cfg, sd, tsd, batches = trainer_case()
    kw = dict(lr=c["lr"], betas=c["betas"], eps=c["eps"], weight_decay=c["weight_decay"], grad_clip=c["grad_clip"],
              accumulate=c["accumulate"], replay_interval=c["replay_interval"], warmup_steps=c["warmup"], total_steps=c["total_steps"],
              task_id=1, teacher_sd={k: v.double() for k, v in tsd.items()},
              spec=R.DistillSpec(modality="balanced", layer_strategy="discounted", gamma=c["gamma"], distillation_coeff=1.0, replay_coeff=1.0))
    kw.update(overrides)
    tr = R.RefTrainer(cfg, {k: v.double() for k, v in sd.items()}, **kw)
    f64 = lambda b: dict(b, patch_embeddings=b["patch_embeddings"].double())
    recs = [tr.step(f64(b), i, f64(m)) for i, (b, m) in enumerate(batches)]
    return {"loss": np.array([r["loss"] for r in recs]), "grad_norm": np.array([r["grad_norm"] for r in recs if "grad_norm" in r]),
            "lr": np.array([r["lr"] for r in recs if "lr" in r]),
            "update": {k: tr.params[k].detach() - sd[k].double() for k in sd}}


def update_errors(got, ref, num_heads):
    """{parameter: rel_err of the update final - initial} of ``got`` against ``ref`` ({name: tensor}; every name of ``ref``).  The
    key third of each query_key_value bias is left out: its gradient is rounding noise (step_parity_errors) that Adam divides by
    eps.  That is H D of each 3 H D bias, below 0.1 % of the parameters; no other element is left out."""
    errs = {}
    for k, r in ref.items():
        a, r = _f64(got[k]), _f64(r)
        assert a.shape == r.shape, (k, a.shape, r.shape)
        if k.endswith("query_key_value.bias"):
            keep = ~key_bias_mask(r.size, num_heads)
            a, r = a[keep], r[keep]
        errs[k] = rel_err(a, r)
    return errs


def check_updates(got, ref, rtol, num_heads, what=""):
    """Every update of update_errors within rtol; the failure names each parameter above the bound.  Returns the largest."""
    errs = update_errors(got, ref, num_heads)
    worst = max(errs, key=errs.get)
    print(f"[rel] {what}: worst update {worst} {errs[worst]:.3e} (bound {rtol:.1e})")
    bad = {k: v for k, v in errs.items() if not v <= rtol}
    assert not bad, f"{what}: update errors above {rtol:.1e}: " + ", ".join(f"{k} {v:.3e}" for k, v in bad.items())
    return errs[worst]
