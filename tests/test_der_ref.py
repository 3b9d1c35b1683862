"""CPU: the float64 restatement of the DER++ head loss (tests/der_ref.py) against torch autograd, its rank rule, and the presence of
the feature's names (the C-ABI pair, the ops wrappers, the plugin) without touching a GPU."""
import os
import re

import pytest
import torch

from tests.der_ref import der_loss, der_ref, gather_targets, rank_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed=0, B=4, T=7, V=24, n_mem=6, A=3):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, T, V, generator=g, dtype=torch.float64) * 3.0
    store = torch.randn(n_mem, A, V, generator=g, dtype=torch.float64) * 3.0
    labels = torch.full((B, T), -100, dtype=torch.int64)
    labels[0, 1:4] = torch.randint(0, V, (3,), generator=g)          # three labelled rows at the front (rows 0, 1, 2)
    labels[1, T - 1] = V - 1                                         # one labelled row, sitting last
    labels[2, 2], labels[2, 5] = 3, 4                                # labelled, unlabelled, unlabelled, labelled: rank != offset
    labels[0, 0] = 5                                                 # (predicted by nothing)
    mem_index = torch.tensor([5, 0, 5, 2])                           # unordered, with a repeat; sample 3 has no label
    return s, store, mem_index, labels


@pytest.mark.parametrize("alpha,beta", [(0.5, 1.0), (1.0, 0.0), (0.0, 1.0), (0.3, 0.7)])
def test_closed_form_gradient_equals_autograd(alpha, beta):
    s, store, mem_index, labels = _case()
    gloss = 1.7
    ref = der_ref(s, store, mem_index, labels, alpha, beta, gloss=gloss)
    x = s.clone().requires_grad_(True)
    loss, ce, mse = der_loss(x, store, mem_index, labels, alpha, beta)
    (gloss * loss).backward()
    assert float((torch.stack([loss, ce, mse]).detach() - ref["out3"]).abs().max()) <= 1e-12
    assert float((x.grad - ref["dlogits"]).abs().max()) <= 1e-12
    assert float(ref["dlogits"][~ref["mask"]].abs().max()) == 0.0 and float(ref["lse"][~ref["mask"]].abs().max()) == 0.0
    assert float(ref["out3"][2]) > 0.0
    # by hand: sample 2 (two labelled rows), the MSE part
    want = (((s[2, 1] - store[5, 0]) ** 2).sum() + ((s[2, 4] - store[5, 1]) ** 2).sum()) / s.shape[-1] / 2.0
    only2 = der_ref(s[2:3], store, mem_index[2:3], labels[2:3], 1.0, 0.0)
    assert abs(float(only2["out3"][0]) - float(want)) <= 1e-12


def test_rank_rule_on_rows_that_are_not_contiguous():
    s, store, mem_index, labels = _case()
    assert rank_map(labels) == [(0, 0, 0), (0, 1, 1), (0, 2, 2), (1, 5, 0), (2, 1, 0), (2, 4, 1)]
    z = gather_targets(store, mem_index, labels)
    assert torch.equal(z[2, 4], store[5, 1]) and torch.equal(z[2, 1], store[5, 0]) and torch.equal(z[0, 2], store[5, 2])
    assert torch.equal(z[1, 5], store[0, 0]) and float(z[3].abs().max()) == 0.0 and float(z[2, 2].abs().max()) == 0.0
    # padding on either side adds -100 labels only: the ranks stay
    # (a label at position 0 is predicted by nothing until something stands in front of it; the VQA batches never label it)
    real = labels.clone()
    real[0, 0] = -100
    padded = torch.nn.functional.pad(real, (2, 3), value=-100)
    assert [(b, t - 2, j) for b, t, j in rank_map(padded)] == rank_map(real) == rank_map(labels)
    # identical student and stored rows: MSE exactly 0, loss = beta CE
    s2 = s.clone()
    for b, t, j in rank_map(labels):
        s2[b, t] = store[int(mem_index[b]), j]
    ref = der_ref(s2, store, mem_index, labels, 0.5, 1.0)
    assert float(ref["out3"][2]) == 0.0 and float(ref["out3"][0]) == float(ref["out3"][1])
    with pytest.raises(IndexError):
        gather_targets(store[:, :2], mem_index, labels)            # sample 0 has three labelled rows
    with pytest.raises(IndexError):
        gather_targets(store, torch.tensor([6, 0, 5, 2]), labels)  # n_mem = 6


def test_der_is_exported_and_not_in_the_registry():
    import mafed_amd
    from mafed_amd import CLMethod, DER, ER
    from mafed_amd.methods import DER as DER2
    assert DER is DER2 and issubclass(DER, ER) and mafed_amd.DER is DER
    assert DER.grads_only_through_model is True
    assert "der" not in CLMethod and len(CLMethod) == 4
    assert CLMethod.names() == list(CLMethod) + ["lwf"]
    assert set(CLMethod) == {"naive", "ewc", "replay", "featdistill"}


def test_new_symbols_are_declared_bound_and_exported():
    from mafed_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "mafed_hip.h")).read()
    lib = _lib.load()
    for name, nargs in (("mafed_ce_mse_fwd", 18), ("mafed_ce_mse_bwd", 16)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/mafed_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert callable(ops.ce_mse_fwd) and callable(ops.ce_mse_bwd)
    tags = [lib.mafed_prof_tag_name(i) for i in range(64)]
    tags = [t.decode() if isinstance(t, bytes) else t for t in tags]
    assert "ce_mse_fwd" in tags and "ce_mse_bwd" in tags
    assert tags.index("ce_mse_bwd") == tags.index("ce_mse_fwd") + 1 and tags[tags.index("ce_mse_bwd") + 1] == "?"


def test_plugin_refuses_a_foreign_model_before_anything_changes():
    import types
    from mafed_amd import DER
    opts = types.SimpleNamespace(tasks=["a", "b"], seed=3, batch_size=2, accumulate_grad_batches=1)
    der = DER(opts, memory_size=4, model_type="vlpythia", alpha=0.3, beta=0.7)
    assert (der.alpha, der.beta) == (0.3, 0.7) and der.logits is None
    ds = {"input_ids": torch.zeros(4, 5, dtype=torch.int64), "attention_mask": torch.ones(4, 5, dtype=torch.int64),
          "labels": torch.full((4, 5), -100, dtype=torch.int64), "patch_embeddings": torch.zeros(4, 2, 3)}
    with pytest.raises(ValueError):
        der.update(ds)
    with pytest.raises(TypeError):
        der.update(ds, model=torch.nn.Linear(2, 2))
    assert der.task_id == 0 and der.mem_dataloader is None and der.datasets == [] and der.logits is None
    sd = der.state_dict()
    assert set(sd) == {"logits", "task_id"}
    der.load_state_dict({"logits": torch.ones(2, 1, 8), "task_id": 2})
    assert der.task_id == 2 and der.logits.shape == (2, 1, 8)
    with pytest.raises(ValueError):
        der.load_state_dict({"task_id": 1})
