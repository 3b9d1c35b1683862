"""PackNet (mafed_amd/methods/packnet.py, csrc/packnet.hip): the mask, hold and view passes and the radix-select prune against the exact
numpy restatement (tests/packnet_ref.py), bit for bit, and the plugin's life inside Trainer.step -- task 0 against Naive, zero forgetting
over three tasks in fp32 and under the bf16 default Trainer with the pipelined optimiser, a checkpoint round trip and the refusals."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import golden_setup, trainer_case
from tests.packnet_ref import hold_ref, mask_ref, prune_ref, select_k, view_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

# 0: empty; 1, 3: scalar tail only; 4: one vector; 15: three vectors and a tail, no group of 16; 16: one group; 17: a group and a tail;
# 1023: less than one block; 4097: several blocks, a group behind them and a tail; 3 * 2^21 + 5: above 2 * 2048 * 256 * 16 / 4, so the
# grid-stride loop at the grid cap goes through its two-group body, its one-group body and the tails
SIZES = [0, 1, 3, 4, 15, 16, 17, 1023, 4097, 3 * 2 ** 21 + 5]
TASK = 1
_INPUTS = {}


def _owner(n, pattern):
    """uint8 owner map with the values {0, 1, 2, 255}: interleaved per element, or in runs of 1 .. 40 elements (so that vectors and groups
    of 16 with no, some and only held elements all occur)."""
    vals = np.array([1, 0, 1, 2, 1, 255], dtype=np.uint8)
    if pattern == "interleaved":
        return vals[np.arange(n) % 6]
    rng = np.random.default_rng(n + 1)
    runs = rng.integers(1, 41, size=n // 8 + 2)
    return np.repeat(vals[np.arange(runs.size) % 6], runs)[:n].copy()


def _inputs(n, pattern):
    """numpy {g, p, anchor, owner, shadow}; g and p carry -0.0, inf and NaN on trainable and on held elements, anchor -0.0, inf and a
    denormal.  Built once per case and left unchanged."""
    key = (n, pattern)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 + n % 997)
        g, p, anchor = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
        for buf, shift in ((g, 0), (p, 1)):
            for j, special in enumerate((-0.0, np.inf, np.nan, -np.inf)):
                buf[(7 * j + shift)::29] = special      # strides coprime to 6: every special meets every owner value
        anchor[3::31] = -0.0
        anchor[4::37] = np.inf
        anchor[5::41] = 3.0e-41
        _INPUTS[key] = dict(g=g, p=p, anchor=anchor, owner=_owner(n, pattern), shadow=rng.integers(0, 2 ** 16, size=n).astype(np.uint16))
    return _INPUTS[key]


def _dev(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).to(DEV)
    return torch.from_numpy(a.copy()).to(DEV)


def _host(t):
    """Device tensor -> numpy with the same bits (bf16 as uint16 patterns)."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    w = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
    return a.shape == b.shape and np.array_equal(a.view(w[a.itemsize]), b.view(w[b.itemsize]))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mask(g_np, owner_np, task):
    from mafed_amd import ops
    g, owner = _dev(g_np), _dev(owner_np)
    nb = ops.packnet_blocks(g.numel())
    part = torch.full((nb + 3,), -7.0, device=DEV)
    ops.packnet_mask_grad_(g, owner, task, part)
    return g, part, nb


@pytest.mark.parametrize("pattern", ["interleaved", "runs"])
@pytest.mark.parametrize("n", SIZES)
def test_packnet_mask_grad(n, pattern):
    from mafed_amd import ops
    x = _inputs(n, pattern)
    g, part, nb = _mask(x["g"], x["owner"], TASK)
    g2, part2, _ = _mask(x["g"], x["owner"], TASK)
    torch.cuda.synchronize()
    assert torch.equal(_bits(part), _bits(part2)) and torch.equal(_bits(g), _bits(g2))     # run to run: the same bits
    assert 1 <= nb <= 2048 and bool((part[nb:] == -7.0).all())
    got, free = _host(g), x["owner"] == TASK
    assert _same_bits(got, mask_ref(x["g"], x["owner"], TASK))
    assert _same_bits(got[free], x["g"][free])                                              # trainable: bit-unchanged, NaN / inf / -0.0 included
    assert _same_bits(got[~free], np.zeros(int((~free).sum()), dtype=np.float32))           # held: +0.0 whatever stood there
    folded = ops.gradnorm_finish(part[:nb], 2.0, torch.empty(2, device=DEV))
    if n == 0:
        assert float(folded[0]) == 0.0 and float(folded[1]) == 1.0
        return
    if bool((~np.isfinite(x["g"][free])).any()):
        assert not np.isfinite(float(folded[0]))        # the trainable inf / NaN are in the norm, as in the one-pass norm of the same buffer
        assert not np.isfinite(float(ops.gradnorm_clip(g, 2.0)[0]))
    # the norm hand-over on a finite gradient: the same buffer with its specials on held elements only (the mask removes them)
    clean = np.where(free & ~np.isfinite(x["g"]), np.float32(0.5), x["g"]).astype(np.float32)
    g, part, nb = _mask(clean, x["owner"], TASK)
    folded = ops.gradnorm_finish(part[:nb], 2.0, torch.empty(2, device=DEV))
    one_pass = ops.gradnorm_clip(g, 2.0)
    ref64 = float(np.sqrt((mask_ref(clean, x["owner"], TASK).astype(np.float64) ** 2).sum()))
    print(f"[packnet] n {n} {pattern}: norm {float(folded[0]):.8g} (one pass {float(one_pass[0]):.8g}, fp64 {ref64:.8g})")
    for i, what in enumerate(("norm", "clip scale")):
        a, b = float(folded[i]), float(one_pass[i])
        assert abs(a - b) <= 1e-6 * abs(b), f"{what}: folded {a} vs one pass {b}"
    assert abs(float(folded[0]) - ref64) <= 1e-6 * ref64


@pytest.mark.parametrize("task", [0, 2, 255])
def test_packnet_mask_grad_other_tasks(task):
    x = _inputs(4097, "runs")
    g, _, _ = _mask(x["g"], x["owner"], task)
    assert _same_bits(_host(g), mask_ref(x["g"], x["owner"], task))


@pytest.mark.parametrize("with_shadow", [True, False], ids=["shadow", "noshadow"])
@pytest.mark.parametrize("pattern", ["interleaved", "runs"])
@pytest.mark.parametrize("n", SIZES)
def test_packnet_hold_and_view(n, pattern, with_shadow):
    from mafed_amd import ops
    x = _inputs(n, pattern)
    owner, anchor = _dev(x["owner"]), _dev(x["anchor"])
    sh_np = x["shadow"] if with_shadow else None
    for task in (TASK, 255):
        p, sh = _dev(x["p"]), (_dev(sh_np) if with_shadow else None)
        ops.packnet_hold_(p, sh, owner, anchor, task)
        want_p, want_sh = hold_ref(x["p"], sh_np, x["owner"], x["anchor"], task)
        got, held = _host(p), x["owner"] != task
        assert _same_bits(got, want_p), f"hold, task {task}"
        assert _same_bits(got[~held], x["p"][~held]) and _same_bits(got[held], x["anchor"][held])
        if with_shadow:
            assert _same_bits(_host(sh), want_sh), f"hold, task {task}: shadow"
            if n:                                       # the rounding is the one ops.cast gives
                cast = _host(ops.cast(anchor, torch.bfloat16))
                assert _same_bits(_host(sh)[held], cast[held]) and _same_bits(_host(sh)[~held], sh_np[~held])
    for k in (0, 1, 2, 255):
        p, sh = _dev(x["p"]), (_dev(sh_np) if with_shadow else None)
        ops.packnet_view_(p, sh, owner, k)
        want_p, want_sh = view_ref(x["p"], sh_np, x["owner"], k)
        assert _same_bits(_host(p), want_p), f"view, k {k}"
        if with_shadow:
            assert _same_bits(_host(sh), want_sh), f"view, k {k}: shadow"
    assert _same_bits(_host(anchor), x["anchor"]) and _same_bits(_host(owner), x["owner"])


def test_packnet_passes_refuse_misaligned_buffers():
    from mafed_amd import _lib, ops
    x = _inputs(1023, "runs")
    g, p, anchor, owner, sh = (_dev(x[k]) for k in ("g", "p", "anchor", "owner", "shadow"))
    part = torch.empty(ops.packnet_blocks(1022), device=DEV)
    seg = torch.tensor([[0, 100]], dtype=torch.int64, device=DEV)
    calls = [lambda: ops.packnet_mask_grad_(g[1:], owner[1:], 1, part), lambda: ops.packnet_mask_grad_(g[4:], owner[4:], 1, part),
             lambda: ops.packnet_hold_(p[1:], sh[1:], owner[1:], anchor[1:], 1), lambda: ops.packnet_hold_(p[4:], None, owner[4:], anchor[4:], 1),
             lambda: ops.packnet_view_(p[2:], sh[2:], owner[2:], 1), lambda: ops.packnet_view_(p[4:], None, owner[4:], 1),
             lambda: ops.packnet_prune_(p[1:], sh[1:], owner[1:], anchor[1:], seg, 1, 1, 0.5)]
    for call in calls:
        with pytest.raises(_lib.MafedHipError):
            call()
    torch.cuda.synchronize()
    for t, k in ((g, "g"), (p, "p"), (anchor, "anchor"), (owner, "owner"), (sh, "shadow")):
        assert _same_bits(_host(t), x[k])


# ---- the selection --------------------------------------------------------------------------------------------------------------------
# One table for every case: length 0, length 1, odd offsets throughout, a segment without a free element (m = 0), 70 001 elements (several
# blocks; several trips at 3 blocks per segment), 2^20 + 3 elements, and a short one that ends the buffer off a vector boundary.
def _segment_table():
    lengths = [0, 1, 70001, 1000, 2 ** 20 + 3, 37]
    segs, off = [], 5
    for length in lengths:
        segs.append((off, length))
        off += length + 3 + (off + length) % 2          # gaps of 3 or 4 elements: the next offset is odd
    return segs, segs[-1][0] + segs[-1][1]              # (the buffer ends with the last segment)


SEGMENTS, N_SEL = _segment_table()
M0_SEGMENT = 3
FAMILIES = ["wide", "shared_top", "low10", "equal", "ties", "special"]
FRACTIONS = [0.0, 0.25, 1.0 / 3.0, 0.5, 1.0]


def _family(name, n, rng):
    """fp32 patterns of the free elements: where the k-th smallest is decided differs by family."""
    if name == "wide":          # all 31 bits random below inf: the top 11 bits spread over every bin
        bits = rng.integers(1 << 20, 0x7F800000, size=n, dtype=np.int64)
    elif name == "shared_top":  # one bin in the first pass; the second and third decide
        bits = (0x3F8 << 20) | rng.integers(0, 1 << 20, size=n, dtype=np.int64)
    elif name == "low10":       # 1 + i 2^-23, i < 1024: one bin in the first two passes
        bits = 0x3F800000 + rng.integers(0, 1024, size=n, dtype=np.int64)
    elif name == "equal":
        bits = np.full(n, 0x3F400000, dtype=np.int64)
    elif name == "ties":        # 40 % 0.5, 20 % 1.0, 40 % 2.0: every fraction's rank lands inside a tie
        bits = np.array([0x3F000000, 0x3F800000, 0x40000000], dtype=np.int64)[rng.choice(3, size=n, p=[0.4, 0.2, 0.4])]
    else:                       # +-0, denormals, normals, +inf, NaN (the signs below make the negatives)
        pool = np.array([0, 0, 1, 0x7FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x7F800001], dtype=np.int64)
        bits = pool[rng.integers(0, pool.size, size=n)]
    sign = rng.integers(0, 2, size=n, dtype=np.int64) << 31
    return (bits | sign).astype(np.uint32).view(np.float32)


_SELECT_INPUTS = {}


def _select_inputs(family):
    """numpy {p, owner, anchor, shadow} over the table: free elements (owner == TASK) from the family; every third element belongs to
    another task (0, 2, 255 in turn) and is smaller in magnitude than any free one (+-0 or a denormal) -- it must be ignored and untouched.
    The gaps between segments hold free elements that no segment covers."""
    if family not in _SELECT_INPUTS:
        rng = np.random.default_rng(FAMILIES.index(family) + 40)
        p = _family(family, N_SEL, rng)
        owner = np.full(N_SEL, TASK, dtype=np.uint8)
        other = np.arange(N_SEL) % 3 == 1
        owner[other] = np.array([0, 2, 255], dtype=np.uint8)[(np.arange(N_SEL) // 3) % 3][other]
        p[other] = np.array([0.0, -0.0, 1e-45, -3e-42], dtype=np.float32)[np.arange(N_SEL) % 4][other]
        off, length = SEGMENTS[M0_SEGMENT]
        owner[off:off + length] = np.where(owner[off:off + length] == TASK, 2, owner[off:off + length])
        anchor = rng.standard_normal(N_SEL).astype(np.float32)
        _SELECT_INPUTS[family] = dict(p=p, owner=owner, anchor=anchor, shadow=rng.integers(1, 2 ** 16, size=N_SEL).astype(np.uint16))
    return _SELECT_INPUTS[family]


def _prune(x, fraction, blocks, with_shadow=True):
    from mafed_amd import ops
    p, owner, anchor = _dev(x["p"]), _dev(x["owner"]), _dev(x["anchor"])
    sh = _dev(x["shadow"]) if with_shadow else None
    seg = torch.tensor(SEGMENTS, dtype=torch.int64, device=DEV)
    stats = ops.packnet_prune_(p, sh, owner, anchor, seg, blocks, TASK, fraction)
    return _host(p), (_host(sh) if with_shadow else None), _host(owner), _host(anchor), _host(stats)


@pytest.mark.parametrize("fraction", FRACTIONS, ids=["f0", "f025", "f033", "f05", "f1"])
@pytest.mark.parametrize("family", FAMILIES)
def test_packnet_prune_is_exact(family, fraction):
    from mafed_amd import ops
    x = _select_inputs(family)
    want = {k: v.copy() for k, v in x.items()}
    want_stats = prune_ref(want["p"], want["shadow"], want["owner"], want["anchor"], SEGMENTS, TASK, fraction)
    default = ops.packnet_select_blocks(max(n for _, n in SEGMENTS), len(SEGMENTS))
    assert default > 3 and 70001 // 4 > 4 * 3 * 256   # 70 001 elements: several blocks in one trip by default, several trips at 3 blocks
    for blocks in (default, 3):
        got = _prune(x, fraction, blocks)
        again = _prune(x, fraction, blocks)
        for name, a, b, c in zip(("p", "shadow", "owner", "anchor", "stats"), got, again,
                                 (want["p"], want["shadow"], want["owner"], want["anchor"], want_stats)):
            assert _same_bits(a, b), f"{name}: two runs differ ({blocks} blocks per segment)"
            assert _same_bits(a, c), f"{name} differs from the restatement ({blocks} blocks per segment)"
    stats = got[4]
    print(f"[packnet] {family} f {fraction:.3f}: m {stats[:, 0].tolist()} k {stats[:, 1].tolist()} pruned {stats[:, 2].tolist()}")
    assert stats[0].tolist() == [0, 0, 0, 0] and stats[M0_SEGMENT].tolist() == [0, 0, 0, 0]
    for (off, length), row in zip(SEGMENTS, stats):
        assert row[1] == select_k(row[0], fraction) and (row[2] >= row[1] if row[1] else row[2] == 0)
    foreign = x["owner"] != TASK
    assert _same_bits(got[0][foreign], x["p"][foreign]) and _same_bits(got[2][foreign], x["owner"][foreign])
    if fraction == 1.0:
        assert stats[4].tolist()[:3] == [stats[4][0]] * 3 and stats[4][0] > 0
    if family == "equal" and fraction > 0:
        assert all(row[2] == row[0] for row in stats if row[1] >= 1)   # every free element is pruned once k >= 1


def test_packnet_prune_without_shadow():
    x = _select_inputs("wide")
    want = {k: v.copy() for k, v in x.items()}
    want_stats = prune_ref(want["p"], None, want["owner"], want["anchor"], SEGMENTS, TASK, 0.5)
    p, _, owner, anchor, stats = _prune(x, 0.5, 7, with_shadow=False)
    assert _same_bits(p, want["p"]) and _same_bits(owner, want["owner"]) and _same_bits(anchor, want["anchor"]) and _same_bits(stats, want_stats)


# ---- plugin level ---------------------------------------------------------------------------------------------------------------------
def _model(cfg, sd, dtype=torch.float32):
    from mafed_amd import VLPythiaConfig, VLPythiaForCausalLM
    mc = VLPythiaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        vision_hidden_size=cfg.vision_hidden_size, num_vision_tokens=cfg.num_vision_tokens)
    m = VLPythiaForCausalLM(mc, compute_dtype=dtype, device=DEV)
    m.load_state_dict(sd, strict=True)
    return m


def _to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _conf(lr=1e-3, grad_norm=2.0):
    return types.SimpleNamespace(accumulate_grad_batches=1, replay_interval=1, grad_norm=grad_norm, learning_rate=lr, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", warmup_steps=0, total_steps=100)


def test_packnet_task0_is_naive(monkeypatch):
    """Three Trainer steps on the trainer_case model in fp32 at the case's clip (2.0, which the gradients exceed): losses, parameters, the
    optimiser's state and the logged norms equal Naive's bit for bit, and the plugin launches nothing.  (The instance promises
    grads_only_through_model while it launches nothing, so the clip norm is collected by the sweep as for Naive; from the prune on it is
    the mask pass's hand-over.)"""
    from mafed_amd import Naive, PackNet, Trainer, ops
    cfg, sd, _, batches = trainer_case()
    res = {}
    for key in ("naive", "packnet"):
        model = _model(cfg, sd)
        method = PackNet() if key == "packnet" else Naive()
        tr = Trainer(model, method, _conf(grad_norm=2.0), task_id=0)
        if key == "packnet":
            for name in ("packnet_mask_grad_", "packnet_hold_"):
                monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("PackNet launched a pass on task 0"))
        recs = [tr.step(_to_dev(batches[i][0]), i) for i in range(3)]
        tr.join()
        torch.cuda.synchronize()
        assert float(tr.optimizer.clip_out[1]) < 1.0    # the clip is at work
        res[key] = [torch.stack([r["loss"] for r in recs]), torch.stack([r["grad_norm"].reshape(()) for r in recs]), model.flat_params.clone()]
        res[key] += [getattr(tr.optimizer, name).clone() for name in tr.optimizer.STATE]
        if key == "packnet":
            assert method.owner is None and method.anchor is None and method.task_id == 0 and model.final_grad_sumsq is None
    assert len(res["naive"]) >= 5
    for a, b in zip(res["packnet"], res["naive"]):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(res["naive"][2], _model(cfg, sd).flat_params)


def _probe(model, batch):
    """Eval-mode logits of a fixed batch."""
    was = model.training
    model.eval()
    with torch.no_grad():
        logits = model(**batch, return_dict=True).logits.clone()
    model.train(was)
    return logits


def _checked_steps(tr, model, pk, batches, first):
    """Trainer steps with the three per-step assertions: in front of the clip the gradient is zero wherever owner != t; the logged norm is
    the float64 norm of that masked gradient at 1e-6; behind the step p == anchor wherever owner != t."""
    seen = {}
    clip = tr.optimizer.clip_grad_norm_

    def clip_and_check(*a, **kw):
        if not pk._all_trainable():
            g = model.flat_grads
            held = pk.owner != pk.task_id
            assert not bool(g[held].view(torch.int32).any()), "a held element has a gradient in front of the clip"
            assert bool(g[~held].any())
            seen["norm"] = float(g.double().norm())
        return clip(*a, **kw)
    tr.optimizer.clip_grad_norm_ = clip_and_check
    for i, b in enumerate(batches):
        seen.clear()
        rec = tr.step(dict(b), first + i)
        tr.join()
        assert rec["stepped"]
        if pk._all_trainable():
            continue
        gn = float(rec["grad_norm"])
        print(f"[packnet] task {pk.task_id} step {first + i}: grad norm {gn:.8g} (fp64 of the masked gradient {seen['norm']:.8g})")
        assert abs(gn - seen["norm"]) <= 1e-6 * seen["norm"]
        held = pk.owner != pk.task_id
        assert torch.equal(_bits(model.flat_params[held]), _bits(pk.anchor[held])), "a held element is off its anchor behind the step"
        if model.flat_shadow is not None:
            assert torch.equal(model.flat_shadow.view(torch.int16), model.flat_params.to(torch.bfloat16).view(torch.int16))
    tr.optimizer.clip_grad_norm_ = clip


def _three_tasks(dtype, stop_after=None):
    """Three tasks of four steps on the smallest golden configuration (t64), each followed by a prune, two retraining steps and update();
    pipelined optimiser, overwriting first sweep, weight decay 0.01.  -> (model, plugin, the probe logits right after each update)."""
    from mafed_amd import PackNet, Trainer
    from oracle import vlpythia_ref as R
    cfg, sd, _, probe, _ = golden_setup("t64")
    probe = _to_dev(probe)
    model = _model(cfg, sd, dtype)
    if dtype == torch.bfloat16:
        model.dw_group_layers = 2
    pk = PackNet(prune_fraction=0.5)
    recorded = []
    for t in range(3):
        batches = [_to_dev(R.make_batch(cfg, 3, 6, seed=700 + 10 * t + i, pad=True, n_answer=3)) for i in range(6)]
        tr = Trainer(model, pk, _conf(lr=2e-3), task_id=t, pipeline_optimizer=True, overwrite_weight_grads=True)
        assert tr._overwrite_ok() == (dtype == torch.bfloat16)
        _checked_steps(tr, model, pk, batches[:4], 0)
        pk.prune(model)
        assert pk.pruned
        _checked_steps(tr, model, pk, batches[4:], 4)
        tr.join()
        pk.update(model)
        assert pk.task_id == t + 1 and not pk.pruned
        recorded.append(_probe(model, probe))
        if stop_after == t:
            break
    torch.cuda.synchronize()
    return model, pk, recorded, probe


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_packnet_zero_forgetting(dtype):
    model, pk, recorded, probe = _three_tasks(dtype)
    report = pk.prune_report(model)
    assert len(report) == 4 * model.config.num_hidden_layers and set(report) == set(pk.prunable_names(model))
    owner = pk.named(model, "owner")
    for name, o in owner.items():
        n, counts = o.numel(), [int((o == t).sum()) for t in range(4)]
        if name not in report:
            assert counts[0] == n                       # never pruned: owner 0 for good
            continue
        # the last prune (task 2): every prune hands on at least floor(m / 2) (ties at tau go too), so m >= n // 4; what it pruned is
        # owned by task 3 now, what it kept by task 2
        row = report[name]
        assert row["m"] >= n // 4 and row["k"] == select_k(row["m"], 0.5) and row["pruned"] >= row["k"] and row["tau_bits"] > 0, (name, row)
        assert sum(counts) == n and counts[3] == row["pruned"] and counts[2] == row["m"] - row["pruned"] and 0 < counts[0] <= n - n // 2, (name, counts)
    p0, sh0 = model.flat_params.clone(), (None if model.flat_shadow is None else model.flat_shadow.clone())
    for k in range(3):
        with pk.task_view(model, k) as m:
            assert m is model
            logits = _probe(model, probe)
            assert not bool(model.flat_params[pk.owner > k].view(torch.int32).any())
        assert torch.equal(_bits(logits), _bits(recorded[k])), f"task {k}: the view's logits differ from those recorded after its update"
        assert torch.equal(_bits(model.flat_params), _bits(p0))                 # leaving the view puts everything back
        if sh0 is not None:
            assert torch.equal(model.flat_shadow.view(torch.int16), sh0.view(torch.int16))
    now = _probe(model, probe)
    assert torch.equal(_bits(now), _bits(recorded[2]))
    assert not torch.equal(now, recorded[0]) and not torch.equal(now, recorded[1]) and not torch.equal(recorded[0], recorded[1])
    with pk.task_view(model, 3):                        # k = the number of finished tasks: the current weights
        assert torch.equal(_bits(_probe(model, probe)), _bits(now))


def test_packnet_state_dict_round_trip_continues_bit_identically():
    from mafed_amd import PackNet, Trainer
    from oracle import vlpythia_ref as R
    model, pk, _, _ = _three_tasks(torch.float32, stop_after=0)
    cfg, sd, _, _, _ = golden_setup("t64")
    sd_pk = pk.state_dict()
    assert set(sd_pk) == {"owner", "anchor", "task_id", "pruned"} and sd_pk["task_id"] == 1 and sd_pk["pruned"] is False
    twin, pk2 = _model(cfg, sd), PackNet(prune_fraction=0.5)
    with torch.no_grad():
        twin.flat_params.copy_(model.flat_params)
    pk2.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd_pk.items()})    # as a checkpoint read on the host gives it
    batches = [_to_dev(R.make_batch(cfg, 3, 6, seed=900 + i, pad=True, n_answer=3)) for i in range(3)]
    out = []
    for m, plugin in ((model, pk), (twin, pk2)):
        tr = Trainer(m, plugin, _conf(lr=2e-3), task_id=1)
        losses = [tr.step(dict(batches[0]), 0)["loss"], tr.step(dict(batches[1]), 1)["loss"]]
        plugin.prune(m)
        losses.append(tr.step(dict(batches[2]), 2)["loss"])
        tr.join()
        torch.cuda.synchronize()
        out.append((torch.stack(losses), m.flat_params.clone(), plugin.owner.clone(), plugin.anchor.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b) if a.dtype == torch.uint8 else torch.equal(_bits(a), _bits(b))
    assert bool((pk2.owner == 2).any()) and pk2.pruned
    with pytest.raises(ValueError, match="pruned"):
        pk2.load_state_dict({"owner": None, "anchor": None, "task_id": 0})
    pk2.load_state_dict({"owner": None, "anchor": None, "task_id": 0, "pruned": False})
    assert pk2.owner is None and pk2.anchor is None and pk2.task_id == 0


def test_packnet_refusals():
    from mafed_amd import PackNet, Trainer
    cfg, sd, _, batch, _ = golden_setup("t64")
    model = _model(cfg, sd)
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, PackNet(), _conf(), ddp=True)
    with pytest.raises(ValueError, match="single-process"):
        Trainer(model, PackNet(), _conf(), reducer=types.SimpleNamespace(world=2))   # a stub: refused before anything looks at it
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="prune_fraction"):
            PackNet(prune_fraction=bad)
    foreign = torch.nn.Linear(2, 2).to(DEV)
    pk = PackNet()

    def enter(m, k=0):
        with pk.task_view(m, k):
            pass
    for call in (lambda: pk.update(foreign), lambda: pk.prune(foreign), lambda: pk.update_after_backward(model=foreign),
                 lambda: pk.update_after_step(model=foreign), lambda: enter(foreign), lambda: pk.prune_report(foreign)):
        with pytest.raises(TypeError, match="native model"):
            call()
    tr = Trainer(model, pk, _conf())
    tr.step(_to_dev(batch), 0)
    pk.prune(model)
    with pytest.raises(RuntimeError, match="pruned already"):
        pk.prune(model)                                 # a second prune in one task
    p0 = model.flat_params.clone()
    with pk.task_view(model, 0):
        with pytest.raises(RuntimeError, match="task_view"):
            tr.step(_to_dev(batch), 1)                  # a step inside a view
        with pytest.raises(RuntimeError, match="nest"):
            enter(model)                                # a nested view
    assert torch.equal(_bits(model.flat_params), _bits(p0))
    with pytest.raises(ValueError, match="task_view"):
        enter(model, 1)                                 # no task has finished yet
    model.zero_grad()
    pk.update(model)
    assert pk.task_id == 1
    pk.task_id = 254                                    # the 255th task is the last a byte-wide map can hold
    owner = pk.owner.clone()
    with pytest.raises(RuntimeError, match="255 tasks"):
        pk.update(model)
    assert pk.task_id == 254 and torch.equal(pk.owner, owner)
