"""``model.head_loss`` (mafed_amd/head_loss.py) with a loss the package does not ship: a caller's own ``HeadLoss`` goes through the dense and
the row-sparse head like the built-in ones."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T, N_ANS = 6, 12, 3   # the fp32 case of the sparse-versus-dense tests: samples with zero, some and N_ANS labelled rows, left padding


def _ragged_batch(cfg, B, T, n_ans, seed):
    """the batch of tests/test_gpu_lwf.py::_ragged_batch"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g)
    am = torch.ones(B, T, dtype=torch.int64)
    labels = torch.full((B, T), -100, dtype=torch.int64)
    for b in range(B):
        k = int(torch.randint(0, n_ans + 1, (1,), generator=g))
        if k:
            labels[b, -k:] = ids[b, -k:]
        am[b, :int(torch.randint(0, 3, (1,), generator=g))] = 0
    feats = torch.randn(B, cfg.num_vision_tokens, cfg.vision_hidden_size, generator=g)
    return {"input_ids": ids.to(DEV), "attention_mask": am.to(DEV), "labels": labels.to(DEV), "patch_embeddings": feats.to(DEV)}


def test_a_callers_own_head_loss_through_the_dense_and_the_sparse_head():
    """``HalfCE``: cross-entropy with the loss and the incoming loss gradient scaled by 0.5.  Dense and with ``max_label_rows``, fp32: loss
    and ``flat_grads`` equal 0.5 x the plain cross-entropy run of the same head within 1e-6 relative (the fp32 bound of the
    sparse-versus-dense tests; the scaling by a power of two is exact, so the bound covers nothing but the order of two launches);
    ``prepare`` saw rows None in the dense run and B * Rc rows in the sparse one, and what it returned came back to ``forward``;
    ``last_head_losses`` is left alone by a loss without parts."""
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    from mafed_amd.head_loss import CrossEntropy
    cfg = VLPythiaConfig(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                         vision_hidden_size=32, num_vision_tokens=8)
    model = VLPythiaForCausalLM(cfg, compute_dtype=torch.float32, device=DEV, seed=5)
    batch = _ragged_batch(cfg, B, T, N_ANS, seed=B + T)
    labelled = (batch["labels"][:, 1:] != -100).sum(1).tolist()
    assert 0 in labelled and N_ANS in labelled and any(0 < k < N_ANS for k in labelled) and int((batch["attention_mask"][:, 0] == 0).sum()) > 0
    seen = []

    class HalfCE(CrossEntropy):
        def prepare(self, feats, input_ids, attention_mask, rows):
            seen.append((None if rows is None else rows.numel(), tuple(input_ids.shape)))
            return len(seen)

        def forward(self, logits, labels, poison, prepared):
            assert prepared == len(seen)
            loss, parts, backward = super().forward(logits, labels, poison, None)
            return loss * 0.5, parts, lambda lg, lab, gl: backward(lg, lab, gl * 0.5)

    def run(hint):
        model.zero_grad()
        kw = {"max_label_rows": hint} if hint is not None else {}
        out = model(**batch, **kw, return_dict=True)
        out.loss.backward()
        torch.cuda.synchronize()
        return float(out.loss.detach()), model.flat_grads.clone()

    marker = model.last_head_losses = torch.full((3,), -7.0, device=DEV)
    plain = [run(None), run(N_ANS)]
    model.head_loss = HalfCE()
    half = [run(None), run(N_ANS)]
    model.head_loss = None
    Rc = N_ANS + 1
    assert seen == [(None, (B, T)), (B * Rc, (B, T))] and B * Rc < B * T, seen
    assert model.last_head_losses is marker and bool((marker == -7.0).all())
    for name, (l0, g0), (l1, g1) in zip(("dense", "max_label_rows"), plain, half):
        assert l0 > 0 and abs(l1 - 0.5 * l0) <= 1e-6 * abs(0.5 * l0), (name, l0, l1)
        rel = float((g1 - 0.5 * g0).norm() / (0.5 * g0).norm())
        print(f"[head_loss] {name}: loss {l0} / {l1}, gradient relative difference to 0.5 x plain {rel:.3e}")
        assert rel <= 1e-6, f"{name}: gradients: relative difference {rel:.3e}"
