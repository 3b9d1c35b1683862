"""CPU guard of the distillation parity bounds (tests/helpers.py): the fp64 oracle against deliberately mutated fp64 oracles must
be rejected by the exact comparators and tolerances that tests/test_gpu_model.py and tests/test_gpu_kernels.py apply to the
native kernels, each by at least GUARD_MARGIN times its bound.  Loosening a bound past what these mutations change fails here."""
import dataclasses

import pytest
import torch

from oracle import vlpythia_ref as R
from tests.helpers import (DISTILL_RTOL, DISTILL_RTOL_BF16, DISTILL_RTOL_INJECT, GUARD_MARGIN, KERNEL_RTOL,
                           LN_INJECT_RTOL, TINY, check_distill_parity, distill_combine_fp64, distill_only_fp64,
                           distill_parity_errors, distill_rows_fp64, distill_variant_cases, g3_spec, golden_setup,
                           ln_injection_fp64, prod_case, rel_err)

MUTATIONS = ("coeff_x1.01", "swap_equal", "drop_layer", "pad_first_valid")


def _first_valid_as_pad(real):
    def masks(attention_mask, P):
        lang, img = real(attention_mask, P)
        lang = lang.clone()
        for b in range(attention_mask.shape[0]):
            nz = torch.nonzero(attention_mask[b]).reshape(-1)
            if nz.numel():
                lang[b, P + int(nz[0])] = 0
        return lang, img
    return masks


def _swapped_weights(real):
    def weights(strategy, lang_mask, img_mask, layer, lang_coeff=None):
        lw, vw = real(strategy, lang_mask, img_mask, layer, lang_coeff)
        return (vw, lw) if strategy == "equal" else (lw, vw)
    return weights


def _dropped_layer(real, k):
    def coeffs(strategy, num_hidden_layers, gamma, distillation_layer):
        layers, c = real(strategy, num_hidden_layers, gamma, distillation_layer)
        c = torch.ones(max(layers) + 1) if c is None else c.clone()   # (distill_loss indexes the coefficients by layer id)
        c[layers[k]] = 0.0
        return layers, c
    return coeffs


def applies(mutation, spec, n_layers):
    if mutation == "swap_equal":
        return spec.modality == "equal"
    if mutation == "pad_first_valid":
        return not spec.cls
    return True


def mutated_oracles(cfg, sd, tsd, batch, spec, monkeypatch):
    """{mutation label: fp64 distillation-only result} for every mutation that applies to ``spec``."""
    n_layers = len(R.layer_coeffs(spec.layer_strategy, cfg.num_hidden_layers - 1, spec.gamma, spec.distillation_layer)[0])
    out = {}
    for m in MUTATIONS:
        if not applies(m, spec, n_layers):
            continue
        for k in (range(n_layers) if m == "drop_layer" else [None]):
            with monkeypatch.context() as mp:
                sp = spec
                if m == "coeff_x1.01":
                    sp = dataclasses.replace(spec, distillation_coeff=spec.distillation_coeff * 1.01)
                elif m == "swap_equal":
                    mp.setattr(R, "modality_weights", _swapped_weights(R.modality_weights))
                elif m == "drop_layer":
                    mp.setattr(R, "layer_coeffs", _dropped_layer(R.layer_coeffs, k))
                else:
                    mp.setattr(R, "modality_masks", _first_valid_as_pad(R.modality_masks))
                out[m if k is None else f"{m}[{k}]"] = distill_only_fp64(cfg, sd, tsd, batch, sp)
    return out


def assert_rejected(mut, ref, rtol, what):
    errs = distill_parity_errors(mut, ref)
    worst = max(errs.values())
    assert worst > GUARD_MARGIN * rtol, f"{what}: mutation moves nothing by more than {worst:.3e} (bound {rtol:.1e})"
    with pytest.raises(AssertionError):
        check_distill_parity(mut, ref, rtol, what)


@pytest.mark.parametrize("name", list(TINY))
def test_model_level_bounds_reject_mutations(name, monkeypatch):
    """test_mafed_distillation_only_vs_fp64_oracle (DISTILL_RTOL) and its combined-loss check (DISTILL_RTOL_INJECT), every
    (config, variant) it runs."""
    cfg, sd, tsd, batch, g = golden_setup(name)
    for n, vname in distill_variant_cases():
        if n != name:
            continue
        spec = g3_spec(vname, cfg, g)
        ref = distill_only_fp64(cfg, sd, tsd, batch, spec)
        muts = mutated_oracles(cfg, sd, tsd, batch, spec, monkeypatch)
        assert "coeff_x1.01" in muts and any(k.startswith("drop_layer") for k in muts)
        for label, mut in muts.items():
            for rtol in (DISTILL_RTOL, DISTILL_RTOL_INJECT):
                assert_rejected(mut, ref, rtol, f"{name}/{vname}/{label}")


def test_production_width_bounds_reject_mutations(monkeypatch):
    """test_distillation_production_width_vs_fp64_oracle: the fp32 bound rejects every mutation.  The bf16 bound (bf16 rounding
    alone moves the gradients by about 1 %) rejects the swapped weights, the misclassified token and the dropped deep layer; the
    1 % coefficient change and dropping layer 0 (the embedding output, whose loss is 1e-3 of layer 1's: 0.8 % of the gradient) are
    below what a bf16 step can resolve and are left to the fp32 check."""
    p = prod_case()
    muts = mutated_oracles(p["cfg"], p["sd"], p["tsd"], p["batch"], p["spec"], monkeypatch)
    assert set(muts) == {"coeff_x1.01", "swap_equal", "drop_layer[0]", "drop_layer[1]", "pad_first_valid"}
    for label, mut in muts.items():
        assert_rejected(mut, p["ref"], DISTILL_RTOL, f"prod fp32/{label}")
        if label not in ("coeff_x1.01", "drop_layer[0]"):
            assert_rejected(mut, p["ref"], DISTILL_RTOL_BF16, f"prod bf16/{label}")


def _kernel_case(h=768, cosine=False):
    g = torch.Generator().manual_seed(5)
    B, P, T = 32, 256, 32
    s = torch.randn(B, P + T, h, generator=g)
    t = s + 0.05 * torch.randn(B, P + T, h, generator=g)
    am = torch.ones(B, T, dtype=torch.int64)
    for b in range(1, B):
        am[b, : int(torch.randint(0, T, (1,), generator=g))] = 0
    am[B // 2] = 0
    return s, t, am, P


@pytest.mark.parametrize("cosine", [False, True])
def test_kernel_bounds_reject_mutations(cosine, monkeypatch):
    """test_distill_production_rows (KERNEL_RTOL on the sums and ds) and test_layernorm_bwd_step_configuration (LN_INJECT_RTOL
    on the injection)."""
    s, t, am, P = _kernel_case(cosine=cosine)
    B, S, h = s.shape
    coef = torch.tensor([3e-4, 5e-5])
    sums, ds = distill_rows_fp64(s, t, am, P, coef, cosine)
    mul = -1.0 if cosine else 2.0 / h
    inj = ln_injection_fp64(s.view(-1, h), t.view(-1, h), am, S, P, coef, mul)

    def rejected(sums_m, ds_m, inj_m, what):
        e_rows = max(rel_err(sums_m[0], sums[0]), rel_err(sums_m[1], sums[1]), rel_err(ds_m, ds))
        assert e_rows > GUARD_MARGIN * KERNEL_RTOL, (what, e_rows)
        assert rel_err(inj_m, inj) > GUARD_MARGIN * LN_INJECT_RTOL, (what, rel_err(inj_m, inj))

    c = coef * 1.01
    rejected(sums, distill_rows_fp64(s, t, am, P, c, cosine)[1], ln_injection_fp64(s.view(-1, h), t.view(-1, h), am, S, P, c, mul), "coef x1.01")
    c = coef.flip(0)
    rejected(sums, distill_rows_fp64(s, t, am, P, c, cosine)[1], ln_injection_fp64(s.view(-1, h), t.view(-1, h), am, S, P, c, mul), "swapped")
    with monkeypatch.context() as mp:
        mp.setattr(R, "modality_masks", _first_valid_as_pad(R.modality_masks))
        sm, dsm = distill_rows_fp64(s, t, am, P, coef, cosine)
        rejected(sm, dsm, ln_injection_fp64(s.view(-1, h), t.view(-1, h), am, S, P, coef, mul), "first valid token as pad")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_combine_bound_rejects_mutations(mode):
    """test_distill_combine (KERNEL_RTOL): coefficient x 1.01, one layer coefficient dropped, lang/vision weights swapped."""
    g = torch.Generator().manual_seed(mode)
    nl = 3
    sums = torch.stack([torch.rand(nl, generator=g) + 0.1, torch.rand(nl, generator=g) + 0.1,
                        torch.full((nl,), 731.0), torch.full((nl,), 8192.0)], dim=1)
    coeff, vec = torch.rand(nl, generator=g) + 0.05, torch.rand(nl, generator=g)
    ref = distill_combine_fp64(sums, coeff, mode, 0.3, vec)

    def worst(out):
        return max(rel_err(a, b) for a, b in zip(out, ref))

    drop = coeff.clone()
    drop[1] = 0.0
    assert worst(distill_combine_fp64(sums, coeff * 1.01, mode, 0.3, vec)) > GUARD_MARGIN * KERNEL_RTOL
    assert worst(distill_combine_fp64(sums, drop, mode, 0.3, vec)) > GUARD_MARGIN * KERNEL_RTOL
    # lang / vision weights swapped: per_layer = vw * lang + lw * vis, injection {c vw / n_lang, c lw / n_vis}
    lang, vis = ref[2][:, 0], ref[2][:, 1]
    lw = (ref[1] - vis) / (lang - vis)
    vw = 1.0 - lw
    per_layer = vw * lang + lw * vis
    inject = torch.stack([coeff.double() * vw / sums[:, 2].double(), coeff.double() * lw / sums[:, 3].double(), ref[3][:, 2], ref[3][:, 3]], 1)
    assert worst(((coeff.double() * per_layer).sum(), per_layer, ref[2], inject)) > GUARD_MARGIN * KERNEL_RTOL
