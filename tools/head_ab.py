#!/usr/bin/env python3
"""Bits of the head losses of one source tree, or of two against each other (run on the GPU box).

    python tools/head_ab.py TREE                  # one "name sha256" line per returned tensor
    python tools/head_ab.py PARENT_TREE BRANCH_TREE > profiles/head_rows_ab.txt      # the lines that differ, then the count

Each tree is a checkout with its library built (TREE/mafed_amd/libmafed_hip.so).  Its package and library are loaded in a fresh child
process of their own -- this process never opens the GPU -- which runs

  * the eight head ops (ce_fwd / ce_bwd, sqnorm_fwd / sqnorm_bwd, ce_kd_fwd / ce_kd_bwd, ce_mse_fwd / ce_mse_bwd) and token_logprob on fp32 and bf16 logits at
    (B, T, V) = (2, 3, 512), (3, 5, 1028) (V % 8 != 0: the narrow bf16 KD kernels), (2, 4, 50304), (5, 66, 512) (a second trip of both
    loops of the finalize kernel) and (1, 1, 512) (no row predicts anything), and on bf16 logits at V = 512 that start 8 bytes past a
    16-byte boundary (the narrow KD kernels at V % 8 == 0); the labels are the full / one / none samples of tests/test_gpu_kd.py in
    their three rotations, with the labels V - 1, 0 and V + 5 in a full sample; poison absent, 0 and 1; tau in {0.5, 1, 2}, lambda in
    {0, 0.3}; for ce_mse a store of A = T rows per sample (the teacher logits) behind a fixed permutation, (alpha, beta) in
    {(0.5, 1), (0, 1), (0.5, 0)};
  * one forward + backward of a tiny model in fp32 and bf16, dense and with ``max_label_rows``, under plain CE, under the squared-norm
    objective, under a logit teacher (LwF after one ``update``) and under a logit anchor (DER++: the store is the model's own
    ``answer_logits`` in a shuffled order, recorded before the parameters move).  The head loss is installed through ``model.head_loss``
    where the tree's model has that slot, else through the three attributes it replaced, so one copy of this script drives both
    trees.  Emitted: the loss, the head's ``dlogits`` as the backward sweep receives them (the ``ops.*_bwd`` wrappers are looked up on the module when the sweep runs) and ``flat_grads``.
    bf16 ``flat_grads`` have been seen to differ from run to run of one tree (give the same tree twice to see which lines do):
    there the loss and ``dlogits`` are the comparison.

The exit status is 0 when every line is equal (or with one tree), 1 when lines differ, 2 when a tree's run failed.
"""
import hashlib
import os
import subprocess
import sys

SHAPES = ((2, 3, 512), (3, 5, 1028), (2, 4, 50304), (5, 66, 512), (1, 1, 512))
KINDS = ("full", "one", "none")


def _labels(torch, B, T, V, first, seed):
    """tests/test_gpu_kd.py::_labels, and in a full sample the labels 0 (T > 2) and V + 5 (T > 3: out of range, counted, row loss 0)"""
    g = torch.Generator().manual_seed(seed)
    labels = torch.full((B, T), -100, dtype=torch.int64)
    for b in range(B):
        kind = KINDS[(first + b) % 3]
        if kind == "full" and T > 1:
            labels[b, 1:] = torch.randint(0, V, (T - 1,), generator=g)
            labels[b, 1] = V - 1
            labels[b, 0] = 5
            if T > 2:
                labels[b, 2] = 0
            if T > 3:
                labels[b, 3] = V + 5
        elif kind == "one":
            labels[b, T - 1] = V - 2
    return labels


def _ragged_batch(torch, cfg, B, T, n_ans, seed, dev):
    """the batch of tests/test_gpu_mas.py::test_sparse_head_equals_dense_head_under_sqnorm"""
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
    return {"input_ids": ids.to(dev), "attention_mask": am.to(dev), "labels": labels.to(dev), "patch_embeddings": feats.to(dev)}


def child(tree):
    sys.path.insert(0, tree)
    import torch
    from mafed_amd import CLMethod, VLPythiaConfig, VLPythiaForCausalLM, _lib, ops
    assert os.path.dirname(os.path.abspath(_lib.LIB_PATH)) == os.path.join(tree, "mafed_amd"), _lib.LIB_PATH
    dev = "cuda"

    def emit(name, t):
        torch.cuda.synchronize()
        raw = t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()
        print(f"{name} {hashlib.sha256(raw).hexdigest()}", flush=True)

    def logits_pair(B, T, V, dtype, seed, offset):
        """student and teacher logits; ``offset``: the student starts 8 bytes (4 bf16 elements) past an allocation's 16-byte boundary"""
        g = torch.Generator().manual_seed(seed)
        s, t = torch.randn(B, T, V, generator=g) * 3.0, torch.randn(B, T, V, generator=g) * 3.0
        s, t = s.to(dev).to(dtype), t.to(dev).to(dtype)
        if offset:
            buf = torch.empty(s.numel() + 4, dtype=dtype, device=dev)
            buf[4:].copy_(s.reshape(-1))
            s = buf[4:].view(B, T, V)
            assert s.data_ptr() % 16 == 8 and s.is_contiguous()
        return s, t

    gl = torch.tensor([1.7], device=dev)
    flags = {"none": None, "0": torch.zeros(1, dtype=torch.int32, device=dev), "1": torch.ones(1, dtype=torch.int32, device=dev)}
    cases = [(shape, dtype, False) for shape in SHAPES for dtype in (torch.float32, torch.bfloat16)] + [((3, 5, 512), torch.bfloat16, True)]
    for (B, T, V), dtype, offset in cases:
        s, t = logits_pair(B, T, V, dtype, 1000 + B * T + V, offset)
        mem_index = torch.randperm(B, generator=torch.Generator().manual_seed(7)).to(dev)   # store = t [B, A = T, V]
        for first in range(3):
            labels = _labels(torch, B, T, V, first, seed=first).to(dev)
            tag = f"{B}x{T}x{V} {str(dtype)[6:]}{' offset' if offset else ''} labels{first}"
            for pname, poison in flags.items():
                loss, lse = ops.ce_fwd(s, labels, poison=poison)
                emit(f"{tag} ce_fwd poison={pname} loss", loss)
                emit(f"{tag} ce_fwd poison={pname} lse", lse)
                J, rowsq = ops.sqnorm_fwd(s, labels, poison=poison)
                emit(f"{tag} sqnorm_fwd poison={pname} J", J)
                emit(f"{tag} sqnorm_fwd poison={pname} rowsq", rowsq)
                out3, lse3 = ops.ce_kd_fwd(s, t, labels, 2.0, 0.3, poison=poison)
                emit(f"{tag} ce_kd_fwd tau=2 lam=0.3 poison={pname} out3", out3)
                emit(f"{tag} ce_kd_fwd tau=2 lam=0.3 poison={pname} lse3", lse3)
                for alpha, beta in ((0.5, 1.0), (0.0, 1.0), (0.5, 0.0)):
                    out3, lse_a = ops.ce_mse_fwd(s, t, mem_index, labels, alpha, beta, poison=poison)
                    emit(f"{tag} ce_mse_fwd alpha={alpha} beta={beta} poison={pname} out3", out3)
                    emit(f"{tag} ce_mse_fwd alpha={alpha} beta={beta} poison={pname} lse", lse_a)
                    if poison is None:
                        emit(f"{tag} ce_mse_bwd alpha={alpha} beta={beta}", ops.ce_mse_bwd(s, t, mem_index, labels, lse_a, alpha, beta, gl))
            emit(f"{tag} ce_bwd", ops.ce_bwd(s, labels, lse, gl))
            emit(f"{tag} sqnorm_bwd", ops.sqnorm_bwd(s, labels, gl))
            for tau in (0.5, 1.0, 2.0):
                for lam in (0.0, 0.3):
                    for name, a, b in ((f"tau={tau} lam={lam}", s, t), (f"tau={tau} lam={lam} student==teacher", s, s)):
                        out3, lse3 = ops.ce_kd_fwd(a, b, labels, tau, lam)
                        emit(f"{tag} ce_kd_fwd {name} out3", out3)
                        emit(f"{tag} ce_kd_fwd {name} lse3", lse3)
                        emit(f"{tag} ce_kd_bwd {name}", ops.ce_kd_bwd(a, b, labels, lse3, tau, lam, gl))
            target = torch.full((B, T), -100, dtype=torch.int64, device=dev)
            target[:, :-1] = labels[:, 1:]
            emit(f"{tag} token_logprob", ops.token_logprob(s.view(B * T, V), target.view(-1)))
            emit(f"{tag} token_logprob scalar loads", ops.token_logprob(s.view(B * T, V)[:, :V - 1], target.view(-1).clamp(max=V - 2)))

    cfg = VLPythiaConfig(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                         vision_hidden_size=32, num_vision_tokens=8)
    seen = []   # what the head's backward returned
    for name in ("ce_bwd", "sqnorm_bwd", "ce_kd_bwd", "ce_mse_bwd"):
        setattr(ops, name, lambda *a, _f=getattr(ops, name), **k: seen.append(_f(*a, **k)) or seen[-1])

    def install(model, sqnorm=False, anchor=None):
        """The head loss of the model's next steps: cross-entropy, the squared norm or an anchor (store, mem_index, alpha, beta)."""
        if hasattr(model, "head_loss"):
            from mafed_amd.head_loss import LogitAnchor, SquaredNorm
            model.head_loss = SquaredNorm() if sqnorm else LogitAnchor(*anchor) if anchor is not None else None
        else:   # a tree from before the slot: three attributes
            model.head_objective, model.logit_teacher, model.logit_anchor = "sqnorm" if sqnorm else "ce", None, anchor

    for dtype, B, T, n_ans in ((torch.float32, 6, 12, 3), (torch.bfloat16, 32, 16, 3)):
        model = VLPythiaForCausalLM(cfg, compute_dtype=dtype, device=dev, seed=5)
        batch = _ragged_batch(torch, cfg, B, T, n_ans, B + T, dev)

        def step(mode):
            for hint in (None, n_ans):
                model.zero_grad()
                del seen[:]
                out = model(**batch, **({"max_label_rows": hint} if hint is not None else {}), return_dict=True)
                out.loss.backward()
                tag = f"step {str(dtype)[6:]} {mode} {'dense' if hint is None else 'max_label_rows'}"
                emit(f"{tag} loss", out.loss)
                assert len(seen) == 1
                emit(f"{tag} dlogits", seen[0])
                emit(f"{tag} flat_grads", model.flat_grads)
                if mode in ("lwf", "der"):
                    emit(f"{tag} last_head_losses", model.last_head_losses)

        step("ce")
        install(model, sqnorm=True)
        step("sqnorm")
        install(model)
        # DER++'s store: the model's own answer logits, sample b in row perm[b] (tests/test_gpu_der.py), before the parameters move
        z = model.answer_logits(batch["patch_embeddings"], batch["input_ids"], batch["attention_mask"], batch["labels"], n_ans)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(dev)
        store = torch.empty_like(z)
        store[perm] = z
        emit(f"step {str(dtype)[6:]} der store", store)
        lwf = CLMethod["lwf"](reg_lambda=1.0, temperature=2.0)
        lwf.update(model)
        gen = torch.Generator(device=dev).manual_seed(6)
        with torch.no_grad():
            model.flat_params.add_(torch.randn(model.flat_params.shape, generator=gen, device=dev) * 1e-2)
        model._shadow_dirty = True
        step("lwf")
        install(model, anchor=(store, perm, 0.5, 1.0))
        step("der")


def run(tree):
    """the lines of a tree, from a fresh process that sees that tree's package and library only"""
    tree = os.path.abspath(tree)
    env = {k: v for k, v in os.environ.items() if k not in ("MAFED_HIP_LIB", "MAFED_HIP_LIB_LOOSE", "PYTHONPATH")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], cwd=tree, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print(f"head_ab: the run of {tree} ended with status {r.returncode}", file=sys.stderr)
        raise SystemExit(2)
    return dict(line.rsplit(" ", 1) for line in r.stdout.splitlines())


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    trees = sys.argv[1:]
    if len(trees) not in (1, 2):
        raise SystemExit(__doc__)
    sides = [run(t) for t in trees]
    if len(sides) == 1:
        for name, h in sides[0].items():
            print(name, h)
        return 0
    a, b = sides
    bad = [n for n in list(a) + [n for n in b if n not in a] if a.get(n) != b.get(n)]
    for n in bad:
        print(f"DIFF  {n}: {a.get(n, 'missing')} / {b.get(n, 'missing')}")
    print(f"head_ab: {len(bad)} of {len(set(a) | set(b))} hashes differ ({trees[0]} / {trees[1]})")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
