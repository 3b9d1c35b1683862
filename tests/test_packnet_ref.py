"""CPU: the numpy / torch restatement of PackNet (tests/packnet_ref.py) against its own algebra -- what tests/test_gpu_packnet.py takes
for exact -- and the importable surface of the plugin."""
import numpy as np
import torch

from tests.packnet_ref import bf16_bits, hold_ref, mag_bits, mask_ref, prune_ref, run_mlp, select_k, view_ref


def test_plugin_surface():
    import mafed_amd
    from mafed_amd.methods import CLMethod, PackNet
    assert mafed_amd.PackNet is PackNet
    pk = PackNet()
    assert pk.prune_fraction == 0.5 and pk.task_id == 0 and pk.pruned is False and pk.owner is None and pk.anchor is None
    assert PackNet.grads_only_through_model is False and PackNet.single_process_only is True
    assert pk.grads_only_through_model is True          # task 0 before its prune: nothing is launched, the instance promises what Naive does
    pk.load_state_dict({"owner": None, "anchor": None, "task_id": 1, "pruned": False})
    assert pk.grads_only_through_model is False
    pk.load_state_dict({"owner": None, "anchor": None, "task_id": 0, "pruned": False})
    assert "packnet" not in CLMethod and len(CLMethod) == 4
    assert pk.state_dict() == {"owner": None, "anchor": None, "task_id": 0, "pruned": False}
    for bad in (-0.1, 1.5):
        try:
            PackNet(prune_fraction=bad)
        except ValueError:
            continue
        raise AssertionError("prune_fraction %r accepted" % bad)


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.0, np.inf, 3.0e-41], dtype=np.float32)
    # a tie goes to the even pattern (down, then up), anything above a tie up; -0, inf and a denormal keep their top halves
    assert bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x8000, 0x7F80, 0x0000]
    got = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bf16_bits(x), got)
    assert (int(bf16_bits(np.array([np.nan], dtype=np.float32))[0]) & 0x7FFF) > 0x7F80


def test_selection_counts():
    rng = np.random.default_rng(5)
    n = 1001
    p = rng.permutation(n).astype(np.float32) + 1.0     # all magnitudes distinct
    p[::2] *= -1.0
    for f in (0.0, 0.25, 1.0 / 3.0, 0.5, 1.0):
        q, owner, anchor = p.copy(), np.zeros(n, dtype=np.uint8), np.ones(n, dtype=np.float32)
        owner[::7] = 3                                   # not free: ignored and untouched
        stats = prune_ref(q, None, owner, anchor, [(0, n)], 0, f)
        m, k = n - len(range(0, n, 7)), select_k(n - len(range(0, n, 7)), f)
        assert stats[0, :3].tolist() == [m, k, k]        # distinct magnitudes: exactly k are pruned
        assert int((owner == 1).sum()) == k and np.array_equal(q[owner == 1], np.zeros(k, dtype=np.float32))
        assert np.array_equal(q[::7], p[::7]) and bool((anchor[::7] == 1.0).all())
        if 0 < k < m:
            assert np.abs(p[owner == 1]).max() < np.abs(p[(owner == 0)]).min()
    assert select_k(10, 1.0 / 3.0) == 3 and select_k(3, 1.0 / 3.0) == 1 and select_k(2, 0.5) == 1 and select_k(0, 0.5) == 0


def test_selection_order_of_patterns():
    p = np.array([-0.0, 0.0, 1e-45, -1e-45, -2.0, 1.0, np.inf, np.nan], dtype=np.float32)
    bits = mag_bits(p)
    assert bits[0] == bits[1] == 0 and bits[2] == bits[3] == 1 and bits[5] < bits[4] < bits[6] < bits[7]
    q, owner, anchor = p.copy(), np.zeros(8, dtype=np.uint8), np.ones(8, dtype=np.float32)
    stats = prune_ref(q, None, owner, anchor, [(0, 8)], 0, 0.375)     # k = 3: tau = the denormal, whose tie is pruned too
    assert stats[0].tolist() == [8, 3, 4, 1] and owner.tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
    assert np.array_equal(q[:4].view(np.uint32), np.zeros(4, dtype=np.uint32))   # +0.0, not -0.0


def test_owned_counts_follow_the_geometric_rule():
    f = 0.5
    pk, _, _, stats = run_mlp(prune_fraction=f)
    for layer, w in enumerate(p for p in pk.params if p.dim() > 1):
        m = w.numel()
        for t in range(3):
            assert stats[t][layer, 0] == m and stats[t][layer, 1] == select_k(m, f) == stats[t][layer, 2]
            m = select_k(m, f)                           # what task t + 1 may train: m f, of which it keeps m f (1 - f)
    owners = np.concatenate([o for o, p in zip(pk.owner, pk.params) if p.dim() > 1])
    total = owners.size
    assert [int((owners == t).sum()) for t in range(4)] == [total // 2, total // 4, total // 8, total // 8]
    for o, p in zip(pk.owner, pk.params):
        if p.dim() == 1:
            assert not o.any()                           # biases: owner 0 for good


def test_task_views_are_bit_identical_after_later_tasks():
    pk, recorded, views, _ = run_mlp(hold=True, weight_decay=0.1)
    for k, (a, b) in enumerate(zip(recorded, views)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"task {k}: the view differs from the model after its update"
    assert not torch.equal(recorded[0], recorded[2])
    # held elements sit on their anchors; pruned slots of the last task are zero in both
    for i, p in enumerate(pk.params):
        flat = p.detach().numpy().reshape(-1)
        assert np.array_equal(flat.view(np.uint32), pk.anchor[i].view(np.uint32))


def test_control_without_the_hold_forgets():
    """Weight decay moves a weight whose gradient is zero: without the hold pass the views drift, so the test above can see a missing one."""
    _, recorded, views, _ = run_mlp(hold=False, weight_decay=0.1)
    assert not torch.equal(recorded[0], views[0]) and not torch.equal(recorded[1], views[1])
    _, recorded, views, _ = run_mlp(hold=False, weight_decay=0.0)     # and it is the decay: without it a masked SGD needs no hold
    assert torch.equal(recorded[0], views[0])


def test_mask_hold_view_touch_only_what_they_should():
    g = np.array([1.0, np.nan, -0.0, np.inf, 5.0], dtype=np.float32)
    owner = np.array([1, 0, 1, 2, 255], dtype=np.uint8)
    out = mask_ref(g, owner, 1)
    assert out.view(np.uint32).tolist() == [0x3F800000, 0, 0x80000000, 0, 0]
    anchor = np.array([9.0, 8.0, 7.0, -0.0, 1.0 + 2.0 ** -8], dtype=np.float32)
    sh = np.full(5, 0x1234, dtype=np.uint16)
    p2, s2 = hold_ref(g, sh, owner, anchor, 1)
    assert p2.view(np.uint32).tolist() == [0x3F800000, 0x41000000, 0x80000000, 0x80000000, anchor.view(np.uint32)[4]]
    assert s2.tolist() == [0x1234, 0x4100, 0x1234, 0x8000, 0x3F80]
    p3, s3 = view_ref(g, sh, owner, 1)
    assert p3.view(np.uint32).tolist() == [0x3F800000, g.view(np.uint32)[1], 0x80000000, 0, 0]   # (the NaN keeps its bits)
    assert s3.tolist() == [0x1234, 0x1234, 0x1234, 0, 0]
