"""Per-layer, per-modality linear CKA of a task sequence's checkpoints (mafed/analysis/get_average_CKA_per_layer.py, without the plots).

    python tools/modality_cka.py --model_dir DIR --batches batches.pt --output_file out.pkl \\
        --run run1/task0.ckpt run1/task1.ckpt ... [--run run2/task0.ckpt ...] [--reference_task 0] [--debiased]

``--model_dir`` holds config.json + weights (VLPythiaForCausalLM.from_pretrained); every ``--run`` lists that run's per-task checkpoints
in task order; ``--batches`` is a torch.save'd list of batch dicts (input_ids, attention_mask, pixel_values or patch_embeddings,
optional rows) -- the data pipeline is not part of this tool.  The output is the reference's pickle, {"image:1".."text:L":
ndarray[n_runs, n_tasks - 1]}, which get_representation_CKA_ratio.py and plot_similarities read.
"""
from __future__ import annotations

import argparse
import os
import pickle
import sys
from typing import Dict, List, Sequence

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def checkpoint_state_dict(ckpt) -> Dict:
    """load_model_from_checkpoint's key handling: the Lightning checkpoint's ["state_dict"] if present, then "model." removed."""
    sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
    return {k.replace("model.", ""): v for k, v in sd.items()}


def stack_runs(per_run: Sequence[Dict[str, Sequence[float]]]) -> Dict[str, np.ndarray]:
    """[{key: values over tasks}] per run -> {key: ndarray[n_runs, n_tasks - 1]} (the reference's cka[key][run, :])."""
    keys = list(per_run[0].keys())
    return {k: np.stack([np.asarray(r[k], dtype=np.float64) for r in per_run]) for k in keys}


def main(argv: List[str] = None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model_dir", required=True)
    ap.add_argument("--run", action="append", nargs="+", required=True, help="one run's per-task checkpoint files, in task order")
    ap.add_argument("--batches", required=True)
    ap.add_argument("--output_file", required=True)
    ap.add_argument("--reference_task", type=int, default=0)
    ap.add_argument("--debiased", action="store_true")
    ap.add_argument("--n_samples", type=int, default=None)
    ap.add_argument("--compute_dtype", choices=("bf16", "fp32"), default="bf16")
    a = ap.parse_args(argv)

    import torch
    from mafed_amd import VLPythiaForCausalLM
    from mafed_amd.analysis import collect_modality_features, modality_cka

    dtype = torch.bfloat16 if a.compute_dtype == "bf16" else torch.float32
    model = VLPythiaForCausalLM.from_pretrained(a.model_dir, compute_dtype=dtype, device="cuda")
    batches = torch.load(a.batches, map_location="cpu")
    per_run = []
    for ckpts in a.run:
        feats = []
        for path in ckpts:
            model.load_state_dict(checkpoint_state_dict(torch.load(path, map_location="cpu")), strict=False)
            feats.append(collect_modality_features(model, batches, a.n_samples))
        cka = modality_cka(feats, reference=a.reference_task, debiased=a.debiased)
        per_run.append({k: v.cpu().numpy() for k, v in cka.items()})
    out = stack_runs(per_run)
    d = os.path.dirname(os.path.abspath(a.output_file))
    os.makedirs(d, exist_ok=True)
    with open(a.output_file, "wb") as fp:
        pickle.dump(out, fp)
    for k, v in out.items():
        print(k, np.array2string(v.mean(0), precision=4))


if __name__ == "__main__":
    main()
