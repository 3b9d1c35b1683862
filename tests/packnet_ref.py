"""A numpy restatement of PackNet's four flat-buffer operations (mafed_amd/csrc/packnet.hip) -- the exact selection by
sorting the 31-bit patterns, the gradient mask, the hold with bf16 round-to-nearest-even, the view -- and a small torch-CPU PackNet over
a plain MLP with masked SGD + weight decay.  Everything here is exact: the GPU tests compare bits."""
import contextlib

import numpy as np
import torch

MAG = np.uint32(0x7FFFFFFF)


def mag_bits(p):
    """The 31-bit pattern of |p|: -0 equals +0, a NaN sorts above +inf."""
    return np.ascontiguousarray(p, dtype=np.float32).view(np.uint32) & MAG


def bf16_bits(x):
    """fp32 -> the bf16 pattern (uint16), round to nearest even; a NaN stays a (quiet) NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def select_k(m, fraction):
    """k = floor(double(fraction) * double(m))."""
    return int(np.floor(np.float64(fraction) * np.float64(m)))


def select_tau(p, owner, task, fraction):
    """One segment -> (m, k, tau): m elements with owner == task, tau = the pattern of the k-th smallest |p| among them (None: k == 0)."""
    free = owner == task
    m = int(free.sum())
    k = select_k(m, fraction)
    if k == 0:
        return m, 0, None
    return m, k, int(np.sort(mag_bits(p)[free], kind="stable")[k - 1])


def prune_ref(p, shadow, owner, anchor, segments, task, fraction):
    """The prune of every segment [(offset, length)], in place on p (fp32), shadow (uint16 patterns or None), owner (uint8), anchor.
    -> int64 [S, 4] = {m, k, pruned, tau}."""
    stats = np.zeros((len(segments), 4), dtype=np.int64)
    for s, (off, length) in enumerate(segments):
        sl = slice(off, off + length)
        m, k, tau = select_tau(p[sl], owner[sl], task, fraction)
        stats[s, :2] = m, k
        if tau is None:
            continue
        hit = (owner[sl] == task) & (mag_bits(p[sl]) <= np.uint32(tau))
        p[sl][hit] = 0.0
        anchor[sl][hit] = 0.0
        owner[sl][hit] = task + 1
        if shadow is not None:
            shadow[sl][hit] = 0
        stats[s, 2:] = int(hit.sum()), tau
    return stats


def mask_ref(g, owner, task):
    """g where owner == task, +0.0 elsewhere (a select: a held inf or NaN leaves no trace)."""
    return np.where(owner == task, g, np.float32(0.0)).astype(np.float32)


def hold_ref(p, shadow, owner, anchor, task):
    """-> (p', shadow'): anchor / bf16(anchor) where owner != task, untouched elsewhere."""
    held = owner != task
    return np.where(held, anchor, p).astype(np.float32), (None if shadow is None else np.where(held, bf16_bits(anchor), shadow).astype(np.uint16))


def view_ref(p, shadow, owner, k):
    """-> (p', shadow'): +0.0 / 0 where owner > k, untouched elsewhere."""
    gone = owner > k
    return np.where(gone, np.float32(0.0), p).astype(np.float32), (None if shadow is None else np.where(gone, np.uint16(0), shadow).astype(np.uint16))


# ---- a torch-CPU PackNet over a plain MLP ------------------------------------------------------------------------------------------
class TorchPackNet:
    """PackNet on ``torch.nn.Sequential`` of Linear layers in fp32 on the CPU: masked SGD with decoupled weight decay
    (p -= lr (g + wd p)), the hold behind it (``hold=False``: the control without it), a per-matrix prune by the exact selection above.
    Biases are never pruned (owner 0 for good)."""

    def __init__(self, net, prune_fraction=0.5, lr=0.05, weight_decay=0.1, hold=True):
        self.net, self.f, self.lr, self.wd, self.hold = net, prune_fraction, lr, weight_decay, hold
        self.params = list(net.parameters())
        self.owner = [np.zeros(p.numel(), dtype=np.uint8) for p in self.params]
        self.anchor = [np.zeros(p.numel(), dtype=np.float32) for p in self.params]
        self.task_id, self.pruned = 0, False

    def _flat(self, i):
        return self.params[i].detach().numpy().reshape(-1)   # (shares the parameter's memory)

    def step(self, x, y):
        self.net.zero_grad()
        loss = torch.nn.functional.mse_loss(self.net(x), y)
        loss.backward()
        t = self.task_id
        with torch.no_grad():
            for i, p in enumerate(self.params):
                g = torch.from_numpy(mask_ref(p.grad.numpy().reshape(-1), self.owner[i], t)).view_as(p)
                p.sub_(self.lr * (g + self.wd * p))
                if self.hold and not (t == 0 and not self.pruned):
                    flat = self._flat(i)
                    flat[:] = hold_ref(flat, None, self.owner[i], self.anchor[i], t)[0]
        return float(loss.detach())

    def prune(self):
        assert not self.pruned
        stats = []
        for i, p in enumerate(self.params):
            if p.dim() > 1:
                flat = self._flat(i)
                stats.append(prune_ref(flat, None, self.owner[i], self.anchor[i], [(0, flat.size)], self.task_id, self.f)[0])
        self.pruned = True
        return np.stack(stats)

    def update(self):
        if not self.pruned:
            self.prune()
        for i in range(len(self.params)):
            self.anchor[i][:] = self._flat(i)
        self.pruned, self.task_id = False, self.task_id + 1

    @contextlib.contextmanager
    def task_view(self, k):
        saved = [self._flat(i).copy() for i in range(len(self.params))]
        try:
            for i in range(len(self.params)):
                flat = self._flat(i)
                flat[:] = view_ref(flat, None, self.owner[i], k)[0]
            yield self.net
        finally:
            for i, s in enumerate(saved):
                self._flat(i)[:] = s


def mlp_case(seed=11, n_tasks=3):
    """(net factory, [(x, y)] per task, probe inputs): a 12-24-24-4 MLP and one regression batch per task."""
    def make():
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(12, 24), torch.nn.ReLU(), torch.nn.Linear(24, 24), torch.nn.ReLU(), torch.nn.Linear(24, 4))
    gen = torch.Generator().manual_seed(seed + 1)
    tasks = [(torch.randn(16, 12, generator=gen), torch.randn(16, 4, generator=gen)) for _ in range(n_tasks)]
    return make, tasks, torch.randn(5, 12, generator=gen)


def run_mlp(hold=True, weight_decay=0.1, prune_fraction=0.5, steps=6, retrain=3):
    """Three tasks of ``steps`` steps, prune, ``retrain`` steps, update.  -> (the plugin, the probe outputs right after each update, the
    probe outputs under task_view(k) after the last task, the prune stats per task)."""
    make, tasks, probe = mlp_case()
    pk = TorchPackNet(make(), prune_fraction=prune_fraction, weight_decay=weight_decay, hold=hold)
    recorded, stats = [], []
    for x, y in tasks:
        for _ in range(steps):
            pk.step(x, y)
        stats.append(pk.prune())
        for _ in range(retrain):
            pk.step(x, y)
        pk.update()
        with torch.no_grad():
            recorded.append(pk.net(probe).clone())
    views = []
    for k in range(len(tasks)):
        with pk.task_view(k), torch.no_grad():
            views.append(pk.net(probe).clone())
    return pk, recorded, views, stats
