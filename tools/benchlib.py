"""The measuring protocol shared by the plugin bench tools (tools/{agem,gem,si,mas,packnet,merge,der,kd,select}_bench.py; DESIGN.md
section 4s): one copy of the compiler's resource table, the device-event timer, the synthetic batch, the Trainer configuration, the step
loops, the A/B against a parent commit's library and the header line.  A tool keeps what is its own: the method it sets up, its kernel
rows with their bytes per parameter, and the labels and marks it prints.

Nothing heavy is imported here: ``--resources`` runs without a GPU before torch loads, and the functions that need torch import it when
they are called.
"""
import datetime
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (column title, its width, the key of the compiler's remark)
_RESOURCE_COLS = (("VGPRs", 6, " VGPRs"), ("SGPRs", 6, "TotalSGPRs"), ("scratch B/lane", 15, r"ScratchSize \[bytes/lane\]"),
                  ("LDS B/block", 12, r"LDS Size \[bytes/block\]"), ("waves/SIMD", 11, r"Occupancy \[waves/SIMD\]"))


def parse_resources(stderr):
    """[(kernel name, (VGPRs, SGPRs, scratch B/lane, LDS B/block, waves/SIMD))] from the -Rpass-analysis=kernel-resource-usage remarks
    of one compile, in the compiler's order; the names demangled and cut down to ``kernel<template arguments>``."""
    out = []
    for block in stderr.split("Function Name: ")[1:]:
        name = subprocess.run(["c++filt", block.split()[0]], capture_output=True, text=True).stdout.strip() or block.split()[0]
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("mafed::", "")
        out.append((name, tuple(re.search(key + r": (\d+)", block).group(1) for _, _, key in _RESOURCE_COLS)))
    return out


def resource_lines(kernels, width, lds=True, renames=(), prefix=""):
    """The table rows of ``parse_resources``' result: the name (``prefix`` in front, each (old, new) of ``renames`` applied) right-aligned
    in ``width``, then the columns, without the LDS one if ``lds`` is false.  The first line is the column titles."""
    keep = [i for i, (title, _, _) in enumerate(_RESOURCE_COLS) if lds or title != "LDS B/block"]
    lines = [" ".join([f"{'kernel':>{width}s}"] + [f"{_RESOURCE_COLS[i][0]:>{_RESOURCE_COLS[i][1]}s}" for i in keep])]
    for name, fields in kernels:
        for old, new in renames:
            name = name.replace(old, new)
        lines.append(" ".join([f"{prefix + name:>{width}s}"] + [f"{fields[i]:>{_RESOURCE_COLS[i][1]}s}" for i in keep]))
    return lines


def resources(sources, width, lds=True, renames=()):
    """Print VGPRs, SGPRs, scratch, LDS and occupancy of every kernel in the ``sources`` (file names under csrc/) as hipcc reports them
    for gfx950.  With more than one source every name carries its ``<src>: `` in front."""
    from mafed_amd import build
    print("# hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage")
    for k, src in enumerate(sources):
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, src), "-o",
                                os.path.join(tmp, "o.o")], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        lines = resource_lines(parse_resources(r.stderr), width, lds, renames, prefix=src + ": " if len(sources) > 1 else "")
        print("\n".join(lines[0 if k == 0 else 1:]))


def timed(fn, reps, warmup=3, before=None):
    """[us per call] of the last ``reps`` of ``warmup + reps`` calls, each between two device events and followed by a synchronise on
    the second; ``before`` runs ahead of every call, outside the events.

    agem, si and mas used to run the warm-up calls back to back and synchronise the device once behind them.  For the measured calls the
    two forms are the same protocol: ``fn`` has run ``warmup`` times before the first of them, the stream is idle when its first event is
    recorded (here because the last warm-up call's second event was waited for, there because of the device synchronise; the tools use
    one stream), and every measured call is treated as before.  What differs is only how the discarded calls are spaced."""
    import torch
    out = []
    for k in range(warmup + reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def rate_row(name, nbytes, us, mark=""):
    """Print one row of a kernel table (median, min, max us, MB, TB/s, ``mark``) and return the TB/s."""
    med = statistics.median(us)
    print(f"{name:>36s} {med:10.1f} {min(us):8.1f} {max(us):8.1f} {nbytes / 1e6:8.1f} {nbytes / med / 1e6:6.2f}{mark}", flush=True)
    return nbytes / med / 1e6


def samples(cfg, n, P, T, gen):
    """``n`` synthetic samples on the CPU from the CPU generator ``gen`` (ids first, then the patch features): T tokens of which the
    last four are labelled, P bf16 patch embeddings, nothing masked.  The caller owns the generator, so successive calls draw on."""
    import torch
    ids = torch.randint(1, cfg.vocab_size, (n, T), generator=gen)
    labels = torch.full((n, T), -100, dtype=torch.int64)
    labels[:, -4:] = ids[:, -4:]
    feats = torch.randn(n, P, cfg.vision_hidden_size, generator=gen).to(torch.bfloat16)
    return {"input_ids": ids, "attention_mask": torch.ones(n, T, dtype=torch.int64), "labels": labels, "patch_embeddings": feats}


def to_dev(batch, sparse_head=False):
    """The batch on the GPU; ``sparse_head`` adds the loader's hint ``max_label_rows = 4``: the row-sparse head (256 of 1024 rows at
    B = 32, T = 32)."""
    batch = {k: v.to("cuda") for k, v in batch.items()}
    if sparse_head:
        batch["max_label_rows"] = 4
    return batch


def step_conf(schedule):
    """The Trainer configuration of the step rows.  ``schedule``: ``"warmup_perc"`` (a tenth of the steps warm up) or ``"no_warmup"``
    (none: the parameters move from step 1, which the tools that consolidate after one step need)."""
    lr = {"warmup_perc": dict(warmup_perc=0.1), "no_warmup": dict(warmup_steps=0, total_steps=100000)}[schedule]
    return types.SimpleNamespace(accumulate_grad_batches=1, replay_interval=1, grad_norm=2.0, learning_rate=5e-5, betas=(0.9, 0.98),
                                 weight_decay=0.01, optim="adamw", **lr)


def run_steps(trainer, batch, steps=12, warmup=4, free=None):
    """(wall ms of each of ``steps`` Trainer.step calls after ``warmup``, every call ending in a device synchronise; free-running ms per
    step of each block, or None; the last step's record).  ``free = (runs, steps)``: blocks of steps with one synchronise behind each
    block -- what a training loop sees, and the form in which the pipelined optimiser runs under the next step's forward.  The step index
    runs on through both phases and every call gets its own copy of ``batch``."""
    import torch
    ts, rec, i = [], None, 0
    for _ in range(warmup + steps):
        t0 = time.perf_counter()
        rec = trainer.step(dict(batch), i)
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
        i += 1
    free_ms = None
    if free is not None:
        free_ms = []
        for _ in range(free[0]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(free[1]):
                rec = trainer.step(dict(batch), i)
                i += 1
            torch.cuda.synchronize()
            free_ms.append((time.perf_counter() - t0) * 1e3 / free[1])
    trainer.join()
    torch.cuda.synchronize()
    return ts, free_ms, rec


def parent_lib_ab(script, parent_lib, child_args=("--naive-only",), rounds=3, *, emit):
    """``script child_args`` with the parent commit's library (``MAFED_HIP_LIB``, loosely bound) and with this tree's, alternating,
    ``rounds`` times, each in a fresh child process; ``emit(who, round, stdout)`` prints a child's result.  Returns 1 at the first child
    that does not exit 0, and starts no further one."""
    parent_lib = os.path.abspath(parent_lib)
    assert os.path.exists(parent_lib), parent_lib
    print("# naive, the parent commit's library against this tree's, alternating, a fresh process each")
    env0 = {k: v for k, v in os.environ.items() if k not in ("MAFED_HIP_LIB", "MAFED_HIP_LIB_LOOSE")}
    for rnd in range(1, rounds + 1):
        for who, env in (("parent library", dict(env0, MAFED_HIP_LIB=parent_lib, MAFED_HIP_LIB_LOOSE="1")), ("this tree's library", env0)):
            r = subprocess.run([sys.executable, os.path.abspath(script), *child_args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                print(f"## {who}, round {rnd}: the run ended with status {r.returncode}", flush=True)
                return 1
            emit(who, rnd, r.stdout)
    return 0


def header(tool_path, argv):
    """``# python tools/<tool> <argv>; HEAD <sha>; <time>``.  (``--head SHA`` in ``argv``: for a tree that was copied to the GPU box
    without its .git.)"""
    head = argv[argv.index("--head") + 1] if "--head" in argv else None
    head = head or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "no git checkout"
    return f"# python {' '.join(['tools/' + os.path.basename(tool_path)] + argv)}; HEAD {head}; {datetime.datetime.now().isoformat(timespec='seconds')}"
