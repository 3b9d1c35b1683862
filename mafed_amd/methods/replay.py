"""Experience replay (reference: mafed/methods/replay.py): a random memory subset per task, plain CE on a memory batch."""
from __future__ import annotations

import numpy as np

from mafed_amd.methods.base import CLStrategy
from mafed_amd.methods.flat import require_native
from mafed_amd.methods.memory import HBMReplayBuffer, dataset_len, take_samples


def make_memory_selection(memory_selection):
    """The plugins' ``memory_selection`` argument: None (random sub-sampling, the reference's), ``"herding"`` / ``"kcenter"`` or a
    ``mafed_amd.selection.MemorySelection``."""
    if memory_selection is None:
        return None
    from mafed_amd.selection import MemorySelection
    if isinstance(memory_selection, str):
        return MemorySelection(memory_selection)
    if not isinstance(memory_selection, MemorySelection):
        raise TypeError(f"memory_selection: expected None, a method name or a MemorySelection, got {type(memory_selection).__name__}")
    return memory_selection


def select_memory_indices(selection, model, dataset, k: int, who: str) -> np.ndarray:
    """The k dataset indices ``selection`` keeps, from the features of ``model`` (the model that just finished the task)."""
    if model is None:
        raise ValueError(f"{who}: memory_selection needs the model that finished the task (update(dataset, model=...))")
    require_native(model, who, "memory_selection reads its pooled hidden states (model.pooled_features)")
    return selection(model, dataset, k)


class ER(CLStrategy):
    grads_only_through_model = True  # every parameter gradient of a step comes out of the model's own backward (Trainer: incremental clip norm)
    def __init__(self, opts, memory_size, model_type, memory_selection=None, **kwargs):
        super().__init__(opts=opts, **{k: v for k, v in kwargs.items() if k in ("reg_lambda", "mask", "scaler")})
        self.memory_size = memory_size
        self.memory_per_task = int(memory_size / (len(opts.tasks) - 1))
        self.datasets = []
        self.rng = np.random.default_rng(opts.seed)
        self.batch_size = opts.batch_size
        self.seed = 1
        self.model_type = model_type
        self.opts = opts
        self.mem_dataloader = None
        self.memory_selection = make_memory_selection(memory_selection)   # None: the reference's random subset

    def update(self, dataset, model=None, **kwargs):
        n = dataset_len(dataset)
        k = min(self.memory_per_task, n)
        if self.memory_selection is None:
            idx = self.rng.choice(np.arange(n), k, replace=False)
        else:   # (raises before anything of the plugin's has changed)
            idx = select_memory_indices(self.memory_selection, model, dataset, k, type(self).__name__)
        self.task_id += 1
        samples = take_samples(dataset, idx, HBMReplayBuffer.KEYS)
        self.datasets.append(samples)
        if self.mem_dataloader is None:
            import torch.distributed as dist
            rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
            dev = model.flat_params.device if model is not None and hasattr(model, "flat_params") else samples["input_ids"].device
            self.mem_dataloader = HBMReplayBuffer(self.batch_size, dev, seed=self.opts.seed, rank=rank, world_size=world)
        self.mem_dataloader.add(samples)

    def update_mask(self, mask=None):
        self.mask = mask

    def compute_loss(self, model, loss, **kwargs):
        return loss

    def replay(self, model):
        batch = next(iter(self.mem_dataloader))
        n_ex = batch["input_ids"].size(0)
        loss = model(**batch, compute_loss=True, return_dict=True).loss
        return loss, n_ex
