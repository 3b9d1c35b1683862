"""GPU: beam search (``generate(num_beams=k)``) over the shared-prefix KV cache against transformers' own beam search
(tests/golden/beam.npz, tools/gen_beam_golden.py), and the three beam kernels (csrc/beam.hip, csrc/attn_decode_beam.hip) plus the 64-row blocks of the
decode layer kernels against their references."""
import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.test_gpu_model import DEV, build_model, close, to_dev
from tools import gen_beam_golden as G

pytestmark = pytest.mark.gpu

EARLY = {False: False, True: True, "never": "never"}


def _case(case):
    g = load_golden("beam.npz")
    eos = int(g[f"{case}/eos"])
    cfg, sd, batch, p = G.case_inputs(case, eos_id=eos if eos >= 0 else None)   # the committed eos id: no oracle run here
    assert p["eos"] == (None if eos < 0 else eos)
    return cfg, sd, batch, p, torch.from_numpy(g[f"{case}/sequences"]), torch.from_numpy(g[f"{case}/scores"]), torch.from_numpy(g[f"{case}/gap"])


def _generate(model, b, p, use_cache, dtype=None):
    pe = b["patch_embeddings"] if dtype is None else b["patch_embeddings"].to(dtype)
    return model.generate(input_ids=b["input_ids"], attention_mask=b["attention_mask"], patch_embeddings=pe, max_new_tokens=p["max_new"],
                          use_cache=use_cache, eos_token_id=p["eos"], pad_token_id=p["eos"], num_beams=p["k"], length_penalty=p["lp"],
                          early_stopping=p["early"], num_return_sequences=p["nrs"], return_dict_in_generate=True)


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("case", list(G.CASES))
def test_beam_generate_fp32_matches_transformers(case, use_cache):
    cfg, sd, batch, p, seqs, scores, gaps = _case(case)
    assert float(gaps.min()) > 1e-4   # no near-tie the fp32 rounding of another implementation could flip
    model = build_model(cfg, sd)
    out = _generate(model, to_dev(batch), p, use_cache)
    assert out.sequences.shape == seqs.shape, (out.sequences.shape, seqs.shape)
    assert torch.equal(out.sequences.cpu(), seqs), (out.sequences.cpu(), seqs)
    close(out.sequences_scores, scores, 1e-4, "sequences_scores")


@pytest.mark.parametrize("case", ["t64_k3_eos", "m64_k3", "t128_k5_eos"])
def test_beam_generate_bf16_cached_equals_recompute(case):
    """bf16: the cached and the recompute paths agree, and both pick the fp32 tokens for every sample whose fixture gap is wide."""
    cfg, sd, batch, p, seqs, scores, gaps = _case(case)
    model = build_model(cfg, sd, dtype=torch.bfloat16)
    b = to_dev(batch)
    oc, ou = _generate(model, b, p, True, torch.bfloat16), _generate(model, b, p, False, torch.bfloat16)
    nrs = p["nrs"]
    wide = [i for i in range(b["input_ids"].shape[0]) if float(gaps[i]) > 5e-2]
    for i in range(b["input_ids"].shape[0]):
        rows = slice(i * nrs, (i + 1) * nrs)
        n = min(oc.sequences.shape[1], ou.sequences.shape[1])
        if torch.equal(oc.sequences[rows, :n], ou.sequences[rows, :n]):
            close(oc.sequences_scores[rows], ou.sequences_scores[rows], 3e-2, f"sample {i}: cached vs recompute scores")
        else:
            assert i not in wide, f"sample {i}: cached and recompute differ where the fp32 gap is {float(gaps[i]):.3e}"
        if i in wide:
            assert torch.equal(oc.sequences[rows, :seqs.shape[1]].cpu(), seqs[rows])
    assert oc.sequences.shape[0] == ou.sequences.shape[0] == seqs.shape[0]


@pytest.mark.parametrize("case", ["t64_k3_eos", "t128_k2_nopad"])
def test_num_beams_one_is_the_greedy_path(case):
    cfg, sd, batch, p, *_ = _case(case)
    model = build_model(cfg, sd)
    b = to_dev(batch)
    kw = dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], patch_embeddings=b["patch_embeddings"], max_new_tokens=p["max_new"],
              eos_token_id=p["eos"])
    for use_cache in (True, False):
        want = model.generate(use_cache=use_cache, **kw)
        assert torch.equal(model.generate(use_cache=use_cache, num_beams=1, **kw), want)
        # return_dict_in_generate is a beam-search option: the greedy path returns its tensor as before
        got = model.generate(use_cache=use_cache, num_beams=1, return_dict_in_generate=True, **kw)
        assert torch.is_tensor(got) and torch.equal(got, want)


def test_greedy_batches_above_64_rows_keep_the_six_launch_layers():
    """The fused layer kernels serve more than 64 rows (64-row blocks) for beam search only: a greedy decode cache of B > 64 stays on
    the six-launch path it used before."""
    from mafed_amd.model import _DecodeCache
    cfg = G.tiny_cfg("t128")
    model = build_model(cfg, G.R.init_weights(cfg, seed=1), dtype=torch.bfloat16)
    n = 3 * cfg.hidden_size
    for B, beams, want in ((64, 1, True), (65, 1, False), (96, 1, False), (32, 3, True), (64, 4, True)):
        S0 = 4
        store = torch.zeros((cfg.num_hidden_layers, B * S0, n), dtype=torch.bfloat16, device=DEV)
        am = torch.ones((B, 2), dtype=torch.int64, device=DEV)
        cache = _DecodeCache(model, list(store.unbind(0)), B, S0, 2, am, prefix_storage=store, beams=beams)
        assert cache.fused is want, (B, beams)


def test_beam_generate_refusals():
    cfg, sd, batch, p, *_ = _case("t64_k2")
    model = build_model(cfg, sd)
    b = to_dev(batch)
    kw = dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], patch_embeddings=b["patch_embeddings"], max_new_tokens=3)
    with pytest.raises(NotImplementedError):
        model.generate(num_beams=2, do_sample=True, **kw)
    with pytest.raises(NotImplementedError):
        model.generate(num_beams=2, use_graph=True, **kw)
    for extra in (dict(num_beam_groups=2), dict(constraints=[object()]), dict(force_words_ids=[[1]])):
        with pytest.raises(NotImplementedError):
            model.generate(num_beams=2, **extra, **kw)
    with pytest.raises(ValueError):
        model.generate(num_beams=2, num_return_sequences=3, **kw)
    with pytest.raises(ValueError):
        model.generate(num_beams=9, **kw)
    for use_cache in (True, False):   # no beam step without a token to generate (both paths refuse alike)
        with pytest.raises(ValueError):
            model.generate(num_beams=2, use_cache=use_cache, **dict(kw, max_new_tokens=0))


@pytest.mark.parametrize("V", [512, 50277, 50304])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_beam_candidates_kernel_equals_log_softmax_topk(V, dt):
    from mafed_amd import ops
    g = torch.Generator().manual_seed(V)
    B = 3
    for k in (1, 2, 3, 5, 8):
        # distinct values where it matters: a random permutation on a fine grid (fp32); in bf16, whose 8-bit mantissa repeats values
        # over 50k entries, a low random floor with 2k + 1 distinct planted values per sample and row above it
        if dt == torch.float32:
            logits = torch.randperm(B * k * V, generator=g).view(B * k, V).float() * (8.0 / (B * k * V))
        else:
            logits = -2.0 - 2.0 * torch.rand(B * k, V, generator=g)
            for row in range(B * k):
                pos = torch.randperm(V, generator=g)[: 2 * k + 1]
                logits[row, pos] = torch.randperm(4 * k + 2, generator=g)[: 2 * k + 1].float() * 0.25 + (row % k) * 0.0625
            logits = logits.to(dt)
        score = -torch.rand(B * k, generator=g) * 0.1
        for kin in sorted({1, k}):
            lg, sc = logits[: B * kin].to(DEV), score[: B * kin].contiguous().to(DEV)
            cs, ct, cp = ops.beam_candidates(lg, sc, B, k)
            acc = (torch.log_softmax(lg.float().cpu().double(), -1) + sc.cpu().double()[:, None]).view(B, kin * V)
            vals, idx = acc.topk(2 * k + 1, dim=-1)
            close(cs, vals[:, :2 * k], 1e-5, f"candidate scores k={k} kin={kin}")
            # every rank whose neighbours are not within fp32 rounding of it holds the same (token, parent) as torch's
            gap = vals[:, :-1] - vals[:, 1:]
            sep = torch.ones(B, 2 * k, dtype=torch.bool)
            sep[:, 1:] &= gap[:, : 2 * k - 1] > 1e-5
            sep &= gap[:, : 2 * k] > 1e-5
            assert bool(sep[:, 0].all() or k == 1 or sep.any()), "test data without separated ranks"
            got = cp.cpu().long() * V + ct.cpu()
            assert torch.equal(got[sep], idx[:, : 2 * k][sep]), (k, kin)


def _rotary(D, S):
    rot = D // 4
    inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    ang = torch.arange(S, dtype=torch.float32)[:, None] * inv[None, :]
    return rot, ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,k,P,T,H,D,cap,t", [(2, 3, 8, 6, 2, 64, 5, 3), (3, 2, 40, 13, 2, 128, 4, 2), (1, 5, 5, 3, 1, 256, 3, 2),
                                                 (2, 8, 8, 6, 2, 64, 4, 0)])
def test_attn_decode_beam_equals_greedy_kernel_on_the_gathered_cache(dt, B, k, P, T, H, D, cap, t):
    """Kernel c against mafed_attn_decode_prerot run once per beam on a cache materialised by gathering the rows through anc."""
    from mafed_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + k * 10 + t)
    S0, n = P + T, 3 * H * D
    rot, cos, sin = _rotary(D, S0 + cap)
    am = torch.ones(B, T, dtype=torch.int64)
    for b in range(B):
        am[b, : (2 * b + 1) % T] = 0   # padded masks
    am = am.to(DEV)
    prefix = torch.randn(B * S0, n, generator=g).to(dt).to(DEV)
    ops.rotate_k_rows_(prefix, B, S0, H, D, rot, cos, sin)
    new = torch.randn(B * k, cap, n, generator=g).to(dt).to(DEV)   # rows < t stand for keys earlier steps stored rotated; row t as written
    anc =torch.zeros(B * k, cap, dtype=torch.int32)
    for b in range(B):
        for r in range(k):
            for j in range(t):
                anc[b * k + r, j] = b * k + int(torch.randint(0, k, (1,), generator=g))
            anc[b * k + r, t] = b * k + r
    anc = anc.to(DEV)
    new_g = new.clone()
    got = ops.attn_decode_beam(prefix, S0, new_g, t, B, k, anc, H, D, rot, cos, sin, am)
    for r in range(k):
        rows = torch.tensor([b * k + r for b in range(B)], device=DEV)
        # materialised per-beam cache: row j of beam r = row j of slot anc[r, j] (row t: the beam's own, still un-rotated)
        mat = torch.stack([torch.stack([new[int(anc[int(s), j]), j] for j in range(cap)]) for s in rows.tolist()])
        want =ops.attn_decode(prefix, S0, mat.contiguous(), t, B, H, D, rot, cos, sin, am, prerot=True)
        close(got.view(B, k, H * D)[:, r].float(), want.float(), 1e-5 if dt == torch.float32 else 2e-2, f"beam {r}")
    # row t of every slot now holds its rotated key, as the greedy kernel leaves it
    assert not torch.equal(new_g[:, t], new[:, t])


@pytest.mark.parametrize("M", [65, 96, 160, 256])
def test_decode_layer_kernels_at_more_rows_equal_64_row_blocks(M):
    """Kernel d: M > 64 rows are 64-row blocks, bit-identical to the separate 64-row launches, and agree with LayerNorm + GEMM."""
    from mafed_amd import ops
    from mafed_amd._lib import EPI_GELU
    h, n1 = 1024, 4096
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, h, generator=g).to(DEV)
    ln = [(1 + 0.1 * torch.randn(h, generator=g)).to(DEV), (0.1 * torch.randn(h, generator=g)).to(DEV),
          (1 + 0.1 * torch.randn(h, generator=g)).to(DEV), (0.1 * torch.randn(h, generator=g)).to(DEV)]
    wqkv = (0.02 * torch.randn(3 * h, h, generator=g)).to(torch.bfloat16).to(DEV)
    bqkv = (0.02 * torch.randn(3 * h, generator=g)).to(DEV)
    w1 = (0.02 * torch.randn(n1, h, generator=g)).to(torch.bfloat16).to(DEV)
    b1 = (0.02 * torch.randn(n1, generator=g)).to(DEV)
    wd = (0.02 * torch.randn(h, h, generator=g)).to(torch.bfloat16).to(DEV)
    w2 = (0.02 * torch.randn(h, n1, generator=g)).to(torch.bfloat16).to(DEV)
    bd, b2 = (0.02 * torch.randn(h, generator=g)).to(DEV), (0.02 * torch.randn(h, generator=g)).to(DEV)
    assert ops.decode_supported(M, h, n1)
    cache = torch.zeros(M, 2, 3 * h, dtype=torch.bfloat16, device=DEV)
    a = ops.decode_ln_qkv_fc1(x, *ln, 1e-5, wqkv, bqkv, cache[:, 1, :], w1, b1)
    ao = torch.randn(M, h, generator=g).to(torch.bfloat16).to(DEV)
    ws = ops.decode_out_workspace(M, h, DEV)
    y = ops.decode_out(x, ao, a, wd, bd, w2, b2, ws)
    for m0 in range(0, M, 64):
        sl = slice(m0, min(M, m0 + 64))
        c2 = torch.zeros(sl.stop - m0, 2, 3 * h, dtype=torch.bfloat16, device=DEV)
        a2 = ops.decode_ln_qkv_fc1(x[sl].contiguous(), *ln, 1e-5, wqkv, bqkv, c2[:, 1, :], w1, b1)
        assert torch.equal(a2, a[sl]) and torch.equal(c2[:, 1], cache[sl, 1])
        ws2 = ops.decode_out_workspace(sl.stop - m0, h, DEV)
        assert torch.equal(ops.decode_out(x[sl].contiguous(), ao[sl].contiguous(), a2, wd, bd, w2, b2, ws2), y[sl])
    ln1, ln2, _, _ = ops.layernorm_fwd(x, *ln, 1e-5, torch.bfloat16, save_stats=False)
    close(cache[:, 1].float(), ops.gemm(ln1, wqkv, False, True, bias=bqkv).float(), 1e-2, "qkv rows")
    close(a.float(), ops.gemm(ln2, w1, False, True, bias=b1, epilogue=EPI_GELU).float(), 1e-2, "gelu(fc1) rows")
    close(y, x + (ao.float() @ wd.float().t() + bd) + (a.float() @ w2.float().t() + b2), 2e-3, "x + dense + fc2")
    assert int(ws[-4 * (h // 32):].view(torch.int32).abs().sum()) == 0


def test_beam_generate_410m_bf16_cached_equals_recompute():
    """VLPythia-410M, B = 32, 256 + 32 tokens, k = 3, bf16.  Random weights make near-ties common, so besides the two paths' outputs
    every cached step is checked against the recompute forward TEACHER-FORCED on the cached path's own beams (rebuilt from its
    candidate lists): the step's top-k scores must agree at bf16 level and its (token, parent) choices wherever the forward's gaps are
    wide.  A wrong ancestry row or a mis-rotated key shows up at the step where it happens, whatever the later steps do."""
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    cfg = VLPythiaConfig.preset("410m", num_vision_tokens=256)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.bfloat16, device=DEV, seed=1234)
    g = torch.Generator().manual_seed(0)
    B, T, k, new = 32, 32, 3, 5
    V = cfg.vocab_size
    ids = torch.randint(1, V, (B, T), generator=g).to(DEV)
    am = torch.ones(B, T, dtype=torch.int64, device=DEV)
    am[1, :5] = 0
    ids[1, :5] = 0
    feats = torch.randn(B, 256, cfg.vision_hidden_size, generator=g).to(torch.bfloat16).to(DEV)
    kw = dict(input_ids=ids, attention_mask=am, patch_embeddings=feats, max_new_tokens=new, eos_token_id=None, num_beams=k,
              return_dict_in_generate=True)
    model.beam_trace = []
    oc = model.generate(use_cache=True, **kw)
    trace, model.beam_trace = model.beam_trace, None
    ou = model.generate(use_cache=False, **kw)
    assert len(trace) == new and oc.sequences.shape == ou.sequences.shape == (B, T + new)
    same = (oc.sequences == ou.sequences).all(1)
    assert float(same.float().mean()) >= 0.75, f"only {int(same.sum())} of {B} rows agree"
    close(oc.sequences_scores[same], ou.sequences_scores[same], 2e-2, "scores of the rows both paths chose")
    # teacher-forced: the beams the cached path ran after step n - 1 (no eos: ranks 0 .. k-1 continue), recomputed in full
    hist = [[[] for _ in range(k)] for _ in range(B)]
    run = torch.zeros(B, k, dtype=torch.float64)
    n_checked = 0
    for n, (cs, ct, cp) in enumerate(trace):
        cs, ct, cp = cs.cpu().double(), ct.cpu(), cp.cpu().long()
        if n > 0:
            seq = torch.tensor([hist[b][r] for b in range(B) for r in range(k)], dtype=torch.int64, device=DEV)
            st = model._engine_forward(feats.repeat_interleave(k, 0), torch.cat([ids.repeat_interleave(k, 0), seq], 1),
                                       torch.cat([am.repeat_interleave(k, 0), torch.ones(B * k, n, dtype=torch.int64, device=DEV)], 1),
                                       None, False, train=False)
            lp = torch.log_softmax(st["logits"][:, -1, :].float(), -1).double().cpu().view(B, k, V) + run[:, :, None]
            vals, idx = lp.view(B, k * V).topk(k + 1, dim=-1)
            # both lists hold the same running scores, so rank by rank they differ by the step's log-probability error alone
            err = float((cs[:, :k] - vals[:, :k]).abs().max())
            assert err < 5e-2, f"step {n}: cached top-{k} scores differ from the teacher-forced recompute by {err:.3e}"
            wide = (vals[:, :k] - vals[:, 1:]).min(1).values > 5e-2   # samples whose top-k order and membership bf16 cannot flip
            got = cp[:, :k] * V + ct[:, :k]
            assert torch.equal(got[wide], idx[wide][:, :k]), f"step {n}: cached choices differ where the recompute's gaps are wide"
            n_checked += int(wide.sum())
        hist = [[hist[b][int(cp[b, r])] + [int(ct[b, r])] for r in range(k)] for b in range(B)]
        run = cs[:, :k].clone()
    assert n_checked > 0, "no wide-gap sample at any step: the choice check compared nothing"
