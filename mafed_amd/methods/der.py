"""Dark Experience Replay, DER++ (Buzzega et al., 2020) for the answer tokens of the VQA batches: experience replay whose memory also
keeps the logits the model gave when a sample was stored.

The reference ships no implementation (its tooling only knows the checkpoint suffix ``_der_``, mafed/utils/eval_utils.py:23), so the
arithmetic is this project's.  Between tasks ``update`` fills the memory like ``ER.update`` and runs the model
that just finished the task over the new samples in inference mode; its logits on their labelled rows go into ``self.logits``
``[N, A, V]`` in the model's compute dtype, slot j of sample n being n's j-th labelled row.  On a replay step one memory batch gives one
student forward and one fused head loss

    loss = beta * CE + alpha * mean_b( sum_t ||s[b,t] - z[m_b, j(b,t)]||^2 / V  /  count_b )

(``csrc/der.hip``: the stored rows are read in place through the batch's ``memory_index``).  The paper draws two memory batches and adds
both terms to a task batch; under the reference's schedule a replay step has no task batch, so one memory batch carries both terms and
the task batches belong to the other steps.  ``beta = 0`` is plain DER, ``alpha = 0`` is ER.  The defaults are the paper's CIFAR values,
untuned here.  Nothing of this plugin has been run on more than one process.
"""
from __future__ import annotations

from typing import Optional

import torch

from mafed_amd.head_loss import LogitAnchor
from mafed_amd.methods.flat import require_native
from mafed_amd.methods.replay import ER


class DER(ER):
    """``ER`` + a store of answer logits beside the replay memory: ``len(self.logits) == len(self.mem_dataloader)``, row n of the store
    belongs to sample n of the buffer.  Constructed directly; not an entry of ``CLMethod``."""
    grads_only_through_model = True  # every parameter gradient of a step comes out of the model's own backward (Trainer: incremental clip norm)

    def __init__(self, opts, memory_size, model_type, alpha: float = 0.5, beta: float = 1.0, memory_selection=None, **kwargs):
        super().__init__(opts, memory_size, model_type, memory_selection=memory_selection, **kwargs)
        self.alpha, self.beta = float(alpha), float(beta)
        self.logits: Optional[torch.Tensor] = None    # [N, A, V] in the recording model's compute dtype
        self.last_ce: Optional[torch.Tensor] = None   # device scalars of the last replay step (no host synchronisation)
        self.last_mse: Optional[torch.Tensor] = None

    # ---- between tasks -----------------------------------------------------------------------------------------------
    def update(self, dataset, model=None, **kwargs):
        """``ER.update``, then the answer logits of the samples it added, from ``model`` (the model that just finished the task)."""
        if model is None:   # (raises before anything of the plugin's has changed)
            raise ValueError("DER: update needs the model that finished the task (update(dataset, model=...))")
        require_native(model, "DER", "the stored logits are its own head's (model.answer_logits) and the replay loss is computed inside its head (model.head_loss)")
        n0 = 0 if self.mem_dataloader is None else len(self.mem_dataloader)
        super().update(dataset, model=model, **kwargs)
        buf = self.mem_dataloader
        buf.attach_index = True   # every batch says which stored samples it drew
        buf._next = None          # (a batch gathered ahead of time carries no index)
        data = {k: v[n0:] for k, v in buf.data.items()}
        n_new = data["input_ids"].shape[0]
        A_new = max(1, int((data["labels"][:, 1:] != -100).sum(dim=1).max().item())) if n_new else 1
        if self.logits is not None and A_new > self.logits.shape[1]:
            # a later task's samples have more labelled rows: the store is laid out again once, the new slots of the earlier samples are zeros
            grown = self.logits.new_zeros((self.logits.shape[0], A_new, self.logits.shape[2]))
            grown[:, : self.logits.shape[1]] = self.logits
            self.logits = grown
        A = A_new if self.logits is None else self.logits.shape[1]
        parts = [] if self.logits is None else [self.logits]
        for lo in range(0, n_new, self.batch_size):
            hi = min(n_new, lo + self.batch_size)
            parts.append(model.answer_logits(data["patch_embeddings"][lo:hi], data["input_ids"][lo:hi], data["attention_mask"][lo:hi],
                                             data["labels"][lo:hi], A))
        self.logits = torch.cat(parts, dim=0)
        assert len(self.logits) == len(buf)

    # ---- inside a step ---------------------------------------------------------------------------------------------------
    def replay(self, model):
        """One memory batch, one student forward: beta CE + alpha MSE against the batch's stored logits (a ``LogitAnchor`` in
        ``model.head_loss`` for that forward).  A model whose slot is taken is refused before anything is launched."""
        if model.head_loss is not None:
            raise ValueError(f"DER: model.head_loss already holds a {type(model.head_loss).__name__} and the replay step needs the slot for "
                             "its LogitAnchor: one head loss per step, not both")
        batch = next(iter(self.mem_dataloader))
        index = batch.pop("memory_index")
        n_ex = batch["input_ids"].size(0)
        model.head_loss = LogitAnchor(self.logits, index, self.alpha, self.beta)
        try:
            loss = model(**batch, compute_loss=True, return_dict=True).loss
        finally:
            model.head_loss = None
        out3 = model.last_head_losses
        self.last_ce, self.last_mse = out3[1], out3[2]
        return loss, n_ex

    # ---- checkpointing -----------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"logits": self.logits, "task_id": self.task_id}

    def load_state_dict(self, sd) -> None:
        missing = [k for k in ("logits", "task_id") if k not in sd]
        if missing:
            raise ValueError("DER state without %s" % missing)
        z = sd["logits"]
        if z is not None:
            if z.dim() != 3:
                raise ValueError(f"DER state: logits must be [N, A, V], got {tuple(z.shape)}")
            dev = self.logits.device if self.logits is not None else (self.mem_dataloader.device if self.mem_dataloader is not None else z.device)
            z = z.detach().to(dev).clone().contiguous()
        self.logits = z
        self.task_id = int(sd["task_id"])
