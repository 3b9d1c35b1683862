"""CPU: the measuring protocol the plugin bench tools share (tools/benchlib.py) -- the resource-table parser and its three formats, the
synthetic batch against the recipe the tools used to write out, the step loops' indices, copies and synchronises, the A/B's order and
environment, and the event timer's call pattern -- all on stubs: no GPU, no compile, no model."""
import os
import sys
import types

import pytest
import torch

from tools import benchlib

REMARKS = """\
csrc/der.hip:35:1: remark: Function Name: _ZN5mafed17ce_mse_fwd_kernelItEEvPKT_S3_PKlS5_iilliPfS6_S6_ [-Rpass-analysis=kernel-resource-usage]
   35 |                                                          float* __restrict__ row_ce, float* __restrict__ row_mse) {
      | ^
csrc/der.hip:35:1: remark:     TotalSGPRs: 44 [-Rpass-analysis=kernel-resource-usage]
csrc/der.hip:35:1: remark:     VGPRs: 31 [-Rpass-analysis=kernel-resource-usage]
csrc/der.hip:35:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
csrc/der.hip:35:1: remark:     ScratchSize [bytes/lane]: 16 [-Rpass-analysis=kernel-resource-usage]
csrc/der.hip:35:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
csrc/der.hip:35:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
csrc/der.hip:35:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
csrc/der.hip:35:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
csrc/der.hip:35:1: remark:     LDS Size [bytes/block]: 32 [-Rpass-analysis=kernel-resource-usage]
In file included from csrc/der.hip:17:
csrc/head_rows.h:95:1: remark: Function Name: _ZN5mafed20head_finalize_kernelILi2EEEvPKfS2_PKliiffPfPKi [-Rpass-analysis=kernel-resource-usage]
csrc/head_rows.h:95:1: remark:     TotalSGPRs: 37 [-Rpass-analysis=kernel-resource-usage]
csrc/head_rows.h:95:1: remark:     VGPRs: 30 [-Rpass-analysis=kernel-resource-usage]
csrc/head_rows.h:95:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
csrc/head_rows.h:95:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
csrc/head_rows.h:95:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
csrc/head_rows.h:95:1: remark:     Occupancy [waves/SIMD]: 5 [-Rpass-analysis=kernel-resource-usage]
csrc/head_rows.h:95:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
csrc/head_rows.h:95:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
csrc/head_rows.h:95:1: remark:     LDS Size [bytes/block]: 4096 [-Rpass-analysis=kernel-resource-usage]
"""


def test_parse_resources_and_the_three_table_formats():
    kernels = benchlib.parse_resources(REMARKS)
    assert kernels == [("ce_mse_fwd_kernel<unsigned short>", ("31", "44", "16", "32", "8")),     # VGPRs, SGPRs, scratch, LDS, waves/SIMD
                       ("head_finalize_kernel<2>", ("30", "37", "0", "4096", "5"))]
    # one source, as gem / packnet / merge / select print it: the bare name
    assert benchlib.resource_lines(kernels, 36) == [
        "%36s %6s %6s %15s %12s %11s" % ("kernel", "VGPRs", "SGPRs", "scratch B/lane", "LDS B/block", "waves/SIMD"),
        "%36s %6s %6s %15s %12s %11s" % ("ce_mse_fwd_kernel<unsigned short>", 31, 44, 16, 32, 8),
        "%36s %6s %6s %15s %12s %11s" % ("head_finalize_kernel<2>", 30, 37, 0, 4096, 5)]
    # der: the source in front, unsigned short spelt bf16
    assert benchlib.resource_lines(kernels, 52, renames=(("unsigned short", "bf16"),), prefix="der.hip: ")[1:] == [
        "%52s %6s %6s %15s %12s %11s" % ("der.hip: ce_mse_fwd_kernel<bf16>", 31, 44, 16, 32, 8),
        "%52s %6s %6s %15s %12s %11s" % ("der.hip: head_finalize_kernel<2>", 30, 37, 0, 4096, 5)]
    # mas: the source in front, no LDS column
    assert benchlib.resource_lines(kernels, 58, lds=False, prefix="mas.hip: ") == [
        "%58s %6s %6s %15s %11s" % ("kernel", "VGPRs", "SGPRs", "scratch B/lane", "waves/SIMD"),
        "%58s %6s %6s %15s %11s" % ("mas.hip: ce_mse_fwd_kernel<unsigned short>", 31, 44, 16, 8),
        "%58s %6s %6s %15s %11s" % ("mas.hip: head_finalize_kernel<2>", 30, 37, 0, 5)]


def _inline_samples(cfg, n, P, T, gcpu):
    """The recipe as si_bench.step_times (and, inside a closure over one generator, gem_bench.step_times) wrote it out."""
    ids = torch.randint(1, cfg.vocab_size, (n, T), generator=gcpu)
    labels = torch.full((n, T), -100, dtype=torch.int64)
    labels[:, -4:] = ids[:, -4:]
    feats = torch.randn(n, P, cfg.vision_hidden_size, generator=gcpu).to(torch.bfloat16)
    return {"input_ids": ids, "attention_mask": torch.ones(n, T, dtype=torch.int64), "labels": labels, "patch_embeddings": feats}


def test_samples_equal_the_inline_recipe_bit_for_bit():
    cfg = types.SimpleNamespace(vocab_size=97, vision_hidden_size=8)
    ours, theirs = torch.Generator().manual_seed(1235), torch.Generator().manual_seed(1235)
    for _ in range(2):      # GEM: the second task's memory draws on from the same generator
        got, want = benchlib.samples(cfg, 6, 5, 7, ours), _inline_samples(cfg, 6, 5, 7, theirs)
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert not torch.equal(got["input_ids"], benchlib.samples(cfg, 6, 5, 7, torch.Generator().manual_seed(1235))["input_ids"])


class _Trainer:
    def __init__(self, log):
        self.log = log

    def step(self, batch, i):
        self.log.append(("step", i, dict(batch)))
        batch["leak"] = i           # must not reach the next call
        return {"i": i}

    def join(self):
        self.log.append(("join",))


def test_run_steps_indices_copies_synchronises_and_one_join(monkeypatch):
    log = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: log.append(("sync",)))
    batch = {"x": 1}
    ts, free, rec = benchlib.run_steps(_Trainer(log), batch, free=(5, 8))
    steps = [e for e in log if e[0] == "step"]
    assert [e[1] for e in steps] == list(range(56)) and all(e[2] == {"x": 1} for e in steps) and batch == {"x": 1}
    assert len(ts) == 12 and len(free) == 5 and all(t >= 0.0 for t in ts + free) and rec == {"i": 55}
    # 16 steps with a synchronise behind each; 5 blocks of a synchronise, 8 steps, a synchronise; one join and the last synchronise
    kinds = [e[0] for e in log]
    assert kinds == ["step", "sync"] * 16 + (["sync"] + ["step"] * 8 + ["sync"]) * 5 + ["join", "sync"]

    del log[:]
    ts, free, rec = benchlib.run_steps(_Trainer(log), batch)
    assert [e[0] for e in log] == ["step", "sync"] * 16 + ["join", "sync"] and [e[1] for e in log if e[0] == "step"] == list(range(16))
    assert len(ts) == 12 and free is None and rec == {"i": 15}


CHILD = """\
import os, sys
count = int(open(sys.argv[1]).read()) + 1
open(sys.argv[1], "w").write(str(count))
if count == int(sys.argv[2]):
    sys.exit(3)
print(count, os.environ.get("MAFED_HIP_LIB", "-"), os.environ.get("MAFED_HIP_LIB_LOOSE", "-"))
"""


def test_parent_lib_ab_order_environment_and_first_failure(tmp_path, monkeypatch, capsys):
    script, lib, counter = tmp_path / "child.py", tmp_path / "parent.so", tmp_path / "count"
    script.write_text(CHILD)
    lib.write_text("")
    monkeypatch.setenv("MAFED_HIP_LIB", "/the/callers/own.so")      # the tree's children must not inherit these
    monkeypatch.setenv("MAFED_HIP_LIB_LOOSE", "1")
    seen = []
    counter.write_text("0")
    rc = benchlib.parent_lib_ab(str(script), str(lib), child_args=(str(counter), "0"), emit=lambda who, rnd, out: seen.append((who, rnd, out.split())))
    assert rc == 0 and counter.read_text() == "6"
    assert seen == [(who, rnd, [str(2 * rnd - 1 + k)] + env) for rnd in (1, 2, 3)
                    for k, (who, env) in enumerate((("parent library", [str(lib), "1"]), ("this tree's library", ["-", "-"])))]
    assert capsys.readouterr().out == "# naive, the parent commit's library against this tree's, alternating, a fresh process each\n"

    del seen[:]
    counter.write_text("0")
    rc = benchlib.parent_lib_ab(str(script), str(lib), child_args=(str(counter), "3"), emit=lambda who, rnd, out: seen.append((who, rnd)))
    assert rc == 1 and counter.read_text() == "3"           # the third child, round 2's first, exits 3: no fourth is started
    assert seen == [("parent library", 1), ("this tree's library", 1)]
    assert capsys.readouterr().out.splitlines()[-1] == "## parent library, round 2: the run ended with status 3"


def test_timed_call_pattern(monkeypatch):
    log = []

    class Event:
        def __init__(self, enable_timing=False):
            assert enable_timing

        def record(self):
            log.append("record")

        def synchronize(self):
            log.append("wait")

        def elapsed_time(self, other):
            log.append("elapsed")
            return 0.002      # ms

    monkeypatch.setattr(torch.cuda, "Event", Event)
    us = benchlib.timed(lambda: log.append("fn"), 4, warmup=2, before=lambda: log.append("before"))
    assert us == [2.0] * 4
    assert log == ["before", "record", "fn", "record", "wait"] * 2 + ["before", "record", "fn", "record", "wait", "elapsed"] * 4
    del log[:]
    assert len(benchlib.timed(lambda: log.append("fn"), 5)) == 5 and log.count("fn") == 8 and "before" not in log


def test_benchlib_imports_nothing_heavy():
    """``--resources`` must work before torch or the kernel library loads."""
    import subprocess
    code = "import sys; sys.path.insert(0, 'tools'); import benchlib; assert 'torch' not in sys.modules and 'mafed_amd' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code], cwd=benchlib.ROOT).returncode == 0


def test_step_conf_has_the_two_schedules_and_nothing_more():
    common = dict(accumulate_grad_batches=1, replay_interval=1, grad_norm=2.0, learning_rate=5e-5, betas=(0.9, 0.98), weight_decay=0.01, optim="adamw")
    assert vars(benchlib.step_conf("warmup_perc")) == dict(common, warmup_perc=0.1)
    assert vars(benchlib.step_conf("no_warmup")) == dict(common, warmup_steps=0, total_steps=100000)
    with pytest.raises(KeyError):
        benchlib.step_conf("cosine")


def test_header_line():
    line = benchlib.header(os.path.join(benchlib.ROOT, "tools", "gem_bench.py"), ["--parent-lib", "x.so", "--head", "abc123"])
    assert line.startswith("# python tools/gem_bench.py --parent-lib x.so --head abc123; HEAD abc123; ")
