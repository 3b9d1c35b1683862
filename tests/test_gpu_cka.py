"""GPU: per-layer, per-modality linear CKA (csrc/cka.hip, mafed_amd.analysis) against the reference's feature_space_linear_cka
(tests/golden/cka.npz), float64 restatements, the in-tree fp32 GEMM, and the golden hidden states."""
import importlib.util
import json
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import vlpythia_ref as R
from tests.helpers import TINY, golden_setup, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3   # tests/test_gpu_model.py's gate for the golden hidden states
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("n_lt_h", "n_gt_h", "hx_ne_hy", "odd_n5_h100", "offset_1e3", "near_identical", "unrelated")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def hsic64(x, y):
    """||(X - mean)^T (Y - mean)||_F^2 in float64 on the CPU."""
    x = x.detach().cpu().double()
    y = y.detach().cpu().double()
    x = x - x.mean(0)
    y = y - y.mean(0)
    return float(((x.T @ y) ** 2).sum())


def np_cka(x, y, debiased=False):
    x = x.astype(np.float64) - x.astype(np.float64).mean(0)
    y = y.astype(np.float64) - y.astype(np.float64).mean(0)
    xy, xx, yy = (np.sum((a.T @ b) ** 2) for a, b in ((x, y), (x, x), (y, y)))
    if not debiased:
        return xy / np.sqrt(xx * yy)
    n = x.shape[0]
    rx, ry = (x * x).sum(1), (y * y).sum(1)

    def deb(t, a, b):
        return t - n / (n - 2.0) * a.dot(b) + a.sum() * b.sum() / ((n - 1) * (n - 2))
    return deb(xy, rx, ry) / np.sqrt(deb(xx, rx, rx) * deb(yy, ry, ry))


# ---- kernel against the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_cka_matches_reference_fixture(name):
    from mafed_amd.analysis import feature_space_linear_cka
    g = load_golden("cka.npz")
    x, y = _t(g[f"case/{name}/x"]), _t(g[f"case/{name}/y"])
    for deb, key in ((False, "cka"), (True, "cka_debiased")):
        v = feature_space_linear_cka(x, y, debiased=deb)
        assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda
        assert abs(float(v) - float(g[f"case/{name}/{key}"])) <= 1e-5, (name, key, float(v), float(g[f"case/{name}/{key}"]))


# ---- properties ----------------------------------------------------------------------------------------------------------------------------
def test_cka_properties():
    from mafed_amd.analysis import feature_space_linear_cka as cka
    gen = torch.Generator().manual_seed(7)
    n, h = 700, 96
    x = torch.randn(n, h, generator=gen)
    y = x @ torch.randn(h, h, generator=gen) * 0.2 + torch.randn(n, h, generator=gen)
    X, Y = x.to(DEV), y.to(DEV)
    base = float(cka(X, Y))
    assert abs(float(cka(X, X)) - 1.0) <= 1e-6
    assert abs(float(cka(X, X, debiased=True)) - 1.0) <= 1e-6
    q, _ = torch.linalg.qr(torch.randn(h, h, generator=gen, dtype=torch.float64))
    assert abs(float(cka((x.double() @ q).float().to(DEV), Y)) - base) <= 1e-5, "orthogonal rotation"
    assert abs(float(cka(X * 3.7, Y)) - base) <= 1e-5, "isotropic scaling"
    off = 1e3 * torch.randn(1, h, generator=gen)
    assert abs(float(cka((x + off).to(DEV), (y - off).to(DEV))) - base) <= 1e-5, "per-column offsets of 1e3"
    assert abs(float(cka(X, Y)) - float(cka(Y, X))) <= 1e-7, "symmetry"
    assert abs(float(cka(X, Y, True)) - float(cka(Y, X, True))) <= 1e-7, "symmetry (debiased)"


def test_hsic_deterministic_and_batch_independent():
    from mafed_amd import ops
    gen = torch.Generator().manual_seed(11)
    sets = [torch.randn(5000, h, generator=gen).to(DEV) * (1 + i) for i, h in enumerate((100, 256, 128, 1))]
    st = [ops.cka_stats(s)[0][0] for s in sets]
    prods = [(sets[0], st[0], sets[0], st[0]), (sets[1], st[1], sets[2], st[2]), (sets[2], st[2], sets[0], st[0]),
             (sets[1], st[1], sets[1], st[1]), (sets[3], st[3], sets[0], st[0])]
    prods = prods * 6   # 30 products: more than one launch's worth
    a = ops.cka_hsic(prods)
    b = ops.cka_hsic(prods)
    singles = torch.cat([ops.cka_hsic([p]) for p in prods])
    assert torch.equal(a, b)
    assert torch.equal(a, singles)
    m1, r1 = ops.cka_stats(sets[1])
    m2, r2 = ops.cka_stats(sets[1])
    assert torch.equal(m1, m2) and torch.equal(r1, r2)


@pytest.mark.parametrize("n", [3, 5, 4099])
@pytest.mark.parametrize("h", [1, 100, 1024])
def test_hsic_tails(n, h):
    from mafed_amd import ops
    gen = torch.Generator().manual_seed(n * 7 + h)
    x = torch.randn(n, h, generator=gen) + 5.0
    y = torch.randn(n, h + 3, generator=gen) - 2.0
    X, Y = x.to(DEV), y.to(DEV)
    (mx, rx), (my, _) = ops.cka_stats(X), ops.cka_stats(Y)
    got = ops.cka_hsic([(X, mx[0], Y, my[0]), (X, mx[0], X, mx[0])]).cpu()
    for g, want in zip(got.tolist(), (hsic64(x, y), hsic64(x, x))):
        assert abs(g - want) <= 1e-5 * abs(want) + 1e-9, (g, want)
    xd = x.double()
    np.testing.assert_allclose(mx[0].cpu().numpy(), xd.mean(0).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(rx[0].cpu().numpy(), ((xd - xd.mean(0)) ** 2).sum(1).numpy(), rtol=1e-10)


def test_hsic_at_410m_width_against_fp64_and_fp32_gemm():
    from mafed_amd import ops
    gen = torch.Generator().manual_seed(3)
    n, h = 16384, 1024
    x = torch.randn(n, h, generator=gen)
    x[:, :4] *= 50.0   # a few large dimensions, as in Pythia's residual stream
    y = 0.5 * x + torch.randn(n, h, generator=gen)
    X, Y = x.to(DEV), y.to(DEV)
    mx, my = ops.cka_stats(X, row_norms=False)[0][0], ops.cka_stats(Y, row_norms=False)[0][0]
    got = ops.cka_hsic([(X, mx, Y, my), (X, mx, X, mx), (Y, my, Y, my)]).cpu().tolist()
    want = [hsic64(x, y), hsic64(x, x), hsic64(y, y)]
    Xc, Yc = (X - X.mean(0)).contiguous(), (Y - Y.mean(0)).contiguous()
    gemm = [float((ops.gemm(a, b, True, False).double() ** 2).sum()) for a, b in ((Xc, Yc), (Xc, Xc), (Yc, Yc))]
    for g, w, q in zip(got, want, gemm):
        assert abs(g - w) <= 1e-5 * w, (g, w)
        assert abs(g - q) <= 1e-5 * w, (g, q)


# ---- pooling ------------------------------------------------------------------------------------------------------------------------------
def _model(cfg, sd, dtype=torch.float32):
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    mc = VLPythiaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        vision_hidden_size=cfg.vision_hidden_size, num_vision_tokens=cfg.num_vision_tokens)
    m = VLPythiaForCausalLM(mc, compute_dtype=dtype, device=DEV)
    m.load_state_dict(sd, strict=True)
    return m


def np_pool(hidden, mask, P):
    """[L][B, S, h] -> [2, L, B, h] by the reference's rules (get_average_CKA_per_layer.py:109-117), float64."""
    out = np.zeros((2, len(hidden), hidden[0].shape[0], hidden[0].shape[2]))
    for i, hs in enumerate(hidden):
        hs = np.asarray(hs, np.float64)
        for b in range(hs.shape[0]):
            t = int(mask[b].sum())
            out[0, i, b] = hs[b, :P].mean(0)
            out[1, i, b] = hs[b, -t:].mean(0)
    return out


@pytest.mark.parametrize("name", list(TINY))
def test_modality_features_match_golden_hidden_states(name):
    cfg, sd, _, batch, g = golden_setup(name)
    model = _model(cfg, sd)
    L, P = cfg.num_hidden_layers, cfg.num_vision_tokens
    b = {k: v.to(DEV) for k, v in batch.items()}
    feats = model.modality_features(b["input_ids"], b["attention_mask"], patch_embeddings=b["patch_embeddings"])
    assert feats.shape == (2, L, batch["input_ids"].shape[0], cfg.hidden_size) and feats.dtype == torch.float32
    want = np_pool([g[f"g1/hidden/{i}"] for i in range(1, L + 1)], batch["attention_mask"].numpy(), P)
    err = np.abs(feats.cpu().double().numpy() - want).max()
    assert err <= TOL * max(1.0, np.abs(want).max()), err
    # against torch pooling of the model's own hidden states (HF hidden_states[1..L], the last one after the final LayerNorm)
    with torch.no_grad():
        hs = model(**b, output_hidden_states=True).hidden_states
    own = np_pool([h.cpu().numpy() for h in hs[1:]], batch["attention_mask"].numpy(), P)
    np.testing.assert_allclose(feats.cpu().double().numpy(), own, rtol=1e-6, atol=1e-6 * np.abs(own).max())
    # a permuted row scatter lands every sample in its row
    B = batch["input_ids"].shape[0]
    rows = torch.tensor([2 * B - 1 - 2 * i for i in range(B)], dtype=torch.int64, device=DEV)
    out = torch.full((2, L, 2 * B, cfg.hidden_size), -7.0, device=DEV)
    model.modality_features(b["input_ids"], b["attention_mask"], patch_embeddings=b["patch_embeddings"], out=out, rows=rows)
    assert torch.equal(out[:, :, rows.cpu()], feats)
    untouched = sorted(set(range(2 * B)) - set(rows.tolist()))
    assert bool((out[:, :, untouched] == -7.0).all())


def test_empty_text_gives_nan():
    from mafed_amd import ops
    B, S, P, T, h = 2, 12, 8, 4, 64
    hs = [torch.randn(B, S, h, device=DEV) for _ in range(2)]
    mask = torch.tensor([[0, 0, 0, 0], [0, 1, 1, 1]], dtype=torch.int64, device=DEV)
    out = torch.zeros(2, 2, B, h, device=DEV)
    ops.cka_pool(hs, mask, P, out)
    assert bool(out[1, :, 0].isnan().all()) and not bool(out[0].isnan().any()) and not bool(out[1, :, 1].isnan().any())
    torch.testing.assert_close(out[1, 1, 1], hs[1][1, -3:].mean(0), rtol=1e-6, atol=1e-6)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("modality_cka_tool", os.path.join(ROOT, "tools", "modality_cka.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_modality_cka_end_to_end(tmp_path):
    from mafed_amd.analysis import collect_modality_features, modality_cka
    cfg, sd, tsd, _, g = golden_setup("t64")
    t = TINY["t64"]
    ckpts = [sd, tsd, R.perturb(sd, seed=77, std=0.05)]
    batches = [R.make_batch(cfg, t["B"], t["T"], seed=300 + i, pad=True) for i in range(4)]
    dbatches = [{k: v.to(DEV) for k, v in bt.items()} for bt in batches]
    L, P = cfg.num_hidden_layers, cfg.num_vision_tokens
    feats, np_feats = [], []
    model = _model(cfg, sd)
    for w in ckpts:
        model.load_state_dict(w, strict=True)
        feats.append(collect_modality_features(model, dbatches))
        per = []
        with torch.no_grad():
            for bt in dbatches:
                hs = model(**bt, output_hidden_states=True).hidden_states
                per.append(np_pool([h.cpu().numpy() for h in hs[1:]], bt["attention_mask"].cpu().numpy(), P))
        np_feats.append(np.concatenate(per, axis=2))
    for deb in (False, True):
        res = modality_cka(feats, reference=1, debiased=deb)
        assert list(res) == [f"image:{i}" for i in range(1, L + 1)] + [f"text:{i}" for i in range(1, L + 1)]
        for m, mod in enumerate(("image", "text")):
            for i in range(L):
                want = [np_cka(np_feats[k][m, i], np_feats[1][m, i], deb) for k in (0, 2)]
                v = res[f"{mod}:{i + 1}"]
                assert v.dtype == torch.float64 and v.shape == (2,)
                np.testing.assert_allclose(v.cpu().numpy(), want, rtol=0, atol=1e-5)
    # the tool: model directory + per-task checkpoint files + saved batches -> the reference's pickle
    mdir = tmp_path / "model"
    mdir.mkdir()
    mc = {"vocab_size": cfg.vocab_size, "hidden_size": cfg.hidden_size, "num_hidden_layers": L, "num_attention_heads": cfg.num_attention_heads,
          "intermediate_size": cfg.intermediate_size, "vision_hidden_size": cfg.vision_hidden_size, "num_vision_tokens": P}
    (mdir / "config.json").write_text(json.dumps(mc))
    torch.save(sd, mdir / "pytorch_model.bin")
    paths = []
    for k, w in enumerate(ckpts):
        p = tmp_path / f"task{k}.ckpt"
        torch.save({"state_dict": {"model." + n: v for n, v in w.items()}}, p)
        paths.append(str(p))
    torch.save(batches, tmp_path / "batches.pt")
    outp = tmp_path / "cka.pkl"
    _tool().main(["--model_dir", str(mdir), "--batches", str(tmp_path / "batches.pt"), "--output_file", str(outp), "--reference_task", "1",
                  "--compute_dtype", "fp32", "--run", *paths, "--run", *paths])
    with open(outp, "rb") as fp:
        table = pickle.load(fp)
    assert list(table) == [f"image:{i}" for i in range(1, L + 1)] + [f"text:{i}" for i in range(1, L + 1)]
    want = modality_cka(feats, reference=1)
    for k, v in table.items():
        assert isinstance(v, np.ndarray) and v.shape == (2, 2) and v.dtype == np.float64
        np.testing.assert_allclose(v, np.stack([want[k].cpu().numpy()] * 2), rtol=0, atol=1e-6)


def test_full_size_410m_self_similarity():
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    from mafed_amd.analysis import collect_modality_features, modality_cka
    B, P, T = 32, 256, 32
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=P)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=DEV, seed=5)
    g = torch.Generator().manual_seed(9)
    am = torch.ones(B, T, dtype=torch.int64)
    for b in range(0, B, 3):
        am[b, : b % 7] = 0
    batch = {"input_ids": torch.randint(1, cfg.vocab_size, (B, T), generator=g).to(DEV), "attention_mask": am.to(DEV),
             "patch_embeddings": torch.randn(B, P, cfg.vision_hidden_size, generator=g).to(torch.bfloat16).to(DEV)}
    f0 = collect_modality_features(model, [batch])
    f1 = collect_modality_features(model, [batch])
    assert f0.shape == (2, cfg.num_hidden_layers, B, cfg.hidden_size)
    assert torch.equal(f0, f1)
    res = modality_cka([f0, f1], reference=0)
    assert len(res) == 2 * cfg.num_hidden_layers
    for k, v in res.items():
        assert v.shape == (1,)
        assert abs(float(v[0]) - 1.0) <= 1e-6, (k, float(v[0]))
