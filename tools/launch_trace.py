"""Host-side launch order of the engine on a tiny three-layer model: for each scenario the (tag, work) sequence of the library's launches
as ``KernelProfile.records()`` reports it.  The order is decided by host code alone, so two checkouts that print the same text launch the
same kernels in the same order with the same problem sizes -- the check for a change that is meant to move code and nothing else
(profiles/engine_split_launch_trace.txt).

    python tools/launch_trace.py              # every scenario
    python tools/launch_trace.py a h          # some (one process each keeps a fault in one from hiding the others)
"""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from mafed_amd import CLMethod, DER, FeatureDistillation, MAS, Naive, Trainer, VLPythiaConfig, VLPythiaForCausalLM
from mafed_amd.profiler import KernelProfile

DEV = "cuda:0"
CFG = dict(vocab_size=512, hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512, vision_hidden_size=32,
           num_vision_tokens=8)


def model(dtype, seed=5):
    m = VLPythiaForCausalLM(VLPythiaConfig(**CFG), compute_dtype=dtype, device=DEV, seed=seed, text_bucket=0)
    assert m.dw_group_layers == 2   # three layers: one full group and one remainder flush
    return m


def batch(B, T, seed, n_answer=3, hint=True):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, CFG["vocab_size"], (B, T), generator=g)
    am = torch.ones(B, T, dtype=torch.int64)
    am[1, :2] = 0   # left padding
    labels = torch.full((B, T), -100, dtype=torch.int64)
    labels[:, -n_answer:] = ids[:, -n_answer:]
    feats = torch.randn(B, CFG["num_vision_tokens"], CFG["vision_hidden_size"], generator=g)
    b = {"input_ids": ids.to(DEV), "attention_mask": am.to(DEV), "labels": labels.to(DEV), "patch_embeddings": feats.to(DEV)}
    if hint:
        b["max_label_rows"] = n_answer
    return b


def conf(accumulate=1):
    return types.SimpleNamespace(accumulate_grad_batches=accumulate, replay_interval=1, grad_norm=2.0, learning_rate=1e-3, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_steps=0, total_steps=100)


def steps(tr, batches):
    for i, b in enumerate(batches):
        tr.step(b, i)
    tr.join()


def train(dtype, B, T, **trainer_kw):
    """Two optimiser steps (the second starts from the state the first left: overwritten matrix gradients, pipelined-update events)."""
    tr = Trainer(model(dtype), Naive(), conf(), task_id=0, **trainer_kw)
    return lambda: steps(tr, [batch(B, T, 11), batch(B, T, 12)])


def scenario_a():   # bf16, 16 * (8 + 24) = 512 rows: grouped weight gradients with fused squares; row-sparse head (16 * 8 slots)
    return train(torch.bfloat16, 16, 24, pipeline_optimizer=True)


def scenario_b():   # bf16, 16 * (8 + 23) = 496 rows: no multiple of the tile
    return train(torch.bfloat16, 16, 23, pipeline_optimizer=True)


def scenario_c():   # fp32, row-sparse head of 4 slots in 10 positions
    return train(torch.float32, 3, 10)


def scenario_d():   # MAFED replay step: fused distillation injecting into two layers
    student, teacher = model(torch.bfloat16), model(torch.bfloat16, seed=6)
    opts = types.SimpleNamespace(tasks=["a", "b"], batch_size=16, seed=1, pin_mem=False, accumulate_grad_batches=1)
    fd = FeatureDistillation(memory_size=10, opts=opts, model_type="vlpythia", num_hidden_layers=2,
                             distillation_modality_weighing_strategy="balanced", distillation_layer_weighing_strategy="discounted",
                             gamma=0.5, distillation_layer=None)
    fd._update_model(teacher)
    fd.task_id = 1
    fd.num_vision_tokens = CFG["num_vision_tokens"]
    fd.mem_dataloader = [batch(16, 24, 21, hint=False)]
    tr = Trainer(student, fd, conf(), task_id=1)
    return lambda: steps(tr, [batch(16, 24, 22, hint=False), batch(16, 24, 23, hint=False)])


def scenario_e():   # LwF: a logit teacher under the row-sparse head, then under the dense one
    m = model(torch.bfloat16)
    lwf = CLMethod["lwf"](reg_lambda=0.7, temperature=2.0)
    lwf.update(m)
    tr = Trainer(m, lwf, conf(), task_id=1)
    return lambda: steps(tr, [batch(16, 24, 31), batch(16, 24, 32, hint=False)])


def scenario_f():   # hidden_grad_taps on two layers
    m = model(torch.bfloat16)
    b = batch(16, 24, 41, hint=False)
    return lambda: m.hidden_grad_taps(b, [0, 2])


def scenario_g():   # a backward beside collectives: ticketed persistent kernels, then the 128 x 128 kernels
    m = model(torch.bfloat16)
    b = batch(16, 24, 51)

    def run():
        for mode in ("ticketed", True):
            m.contended_backward = mode
            m(**b, return_dict=True).loss.backward()
        m.contended_backward = False
    return run


def scenario_h():   # generate over a shared-image prefill, one score call
    m = model(torch.bfloat16).eval()
    b = batch(4, 6, 61, hint=False)
    idx = torch.tensor([0, 0, 1, 1], device=DEV)
    kw = dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], patch_embeddings=b["patch_embeddings"][:2].contiguous(), image_index=idx)
    cand = torch.randint(1, CFG["vocab_size"], (4, 3, 4), generator=torch.Generator().manual_seed(62)).to(DEV)

    def run():
        m.generate(max_new_tokens=4, eos_token_id=None, **kw)
        m.score(candidate_ids=cand, **kw)
    return run


def scenario_i():   # DER++: one replay step (the memory batch under the row-sparse head) after update
    m = model(torch.bfloat16)
    opts = types.SimpleNamespace(tasks=["a", "b"], seed=11, batch_size=16, accumulate_grad_batches=1)
    der = DER(opts, memory_size=16, model_type="vlpythia")
    der.update({k: v.cpu() for k, v in batch(16, 24, 71, hint=False).items()}, model=m)
    tr = Trainer(m, der, conf(), task_id=1)
    return lambda: steps(tr, [batch(16, 24, 72)])


def scenario_j():   # MAS: the importance pass over two batches, consolidation, then one step with the penalty
    m = model(torch.bfloat16)
    mas = MAS(reg_lambda=4.0)
    tr = Trainer(m, mas, conf(), task_id=0)
    loader = [batch(16, 24, 81), batch(16, 24, 82, hint=False)]

    def run():
        mas.update(m, dataloader=loader)
        steps(tr, [batch(16, 24, 83)])
    return run


SCENARIOS = {f[len("scenario_"):]: v for f, v in sorted(globals().items()) if f.startswith("scenario_")}


def main(names):
    for name in names or list(SCENARIOS):
        run = SCENARIOS[name]()
        torch.cuda.synchronize()
        with KernelProfile() as prof:
            run()
        print(f"## scenario {name}: {SCENARIOS[name].__doc__ or ''}".rstrip(": "))
        for tag, work, _ in prof.records():
            print(f"{tag} {work:.6g}")
        sys.stdout.flush()


if __name__ == "__main__":
    main(sys.argv[1:])
