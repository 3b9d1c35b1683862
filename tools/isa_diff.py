#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel (needs hipcc, no GPU).

    python tools/isa_diff.py PARENT_TREE BRANCH_TREE [--keep DIR]

Every mafed_amd/csrc/*.hip of both trees is compiled to device assembly with build.py's FLAGS, split by function and
normalised (comments, .file / .ident lines and the function index of local labels dropped; names demangled with the
anonymous namespace removed), so that a kernel which only moved between files compares equal.  Per function the
instruction text and the register / scratch / LDS sizes of its kernel descriptor are compared.  Prints one line per
differing kernel, then a count; the exit status is 0 only when every kernel is identical.  --keep DIR keeps the
assembly there and reuses what is newer than its sources.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

DESC_FIELDS = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_accum_offset", ".amdhsa_private_segment_fixed_size",
               ".amdhsa_group_segment_fixed_size")
MANGLED = re.compile(r"_Z[A-Za-z0-9_$.]+")


def _build_py(tree):
    spec = importlib.util.spec_from_file_location("_mafed_build", os.path.join(tree, "mafed_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(tree, out):
    """csrc/*.hip of `tree` -> out/*.s; returns the paths."""
    b = _build_py(tree)
    csrc = os.path.join(tree, "mafed_amd", "csrc")
    deps = glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(tree, "include", "mafed_hip.h")]
    os.makedirs(out, exist_ok=True)
    jobs = [(s, os.path.join(out, os.path.basename(s)[:-4] + ".s")) for s in sorted(glob.glob(os.path.join(csrc, "*.hip")))]
    for stale in set(glob.glob(os.path.join(out, "*.s"))) - {o for _, o in jobs}:
        os.remove(stale)

    def cc(job):
        s, o = job
        if os.path.exists(o) and all(os.path.getmtime(p) < os.path.getmtime(o) for p in [s] + deps):
            return
        r = subprocess.run([b._hipcc()] + b.FLAGS + ["--cuda-device-only", "-S", s, "-o", o], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (s, r.stderr[-4000:]))

    with cf.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(cc, jobs))
    return [o for _, o in jobs]


def demangle(names):
    names = sorted(names)
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt or not names:
        return {n: n.replace("12_GLOBAL__N_1", "") for n in names}
    out = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: d.replace("(anonymous namespace)::", "") for n, d in zip(names, out)}


def functions(paths):
    """{demangled name: (instruction text, descriptor fields)} over all files."""
    raw = {}
    for path in paths:
        name, typed, body, desc, in_desc = None, "", [], {}, False
        for line in open(path):
            line = line.split(";", 1)[0].rstrip()
            if not line.strip():
                continue
            if name is None:
                m = re.match(r"^\s*\.type\s+(\S+),@function$", line)
                if m:
                    typed = m.group(1)
                elif line == typed + ":":
                    name, body, desc = typed, [], {}
                continue
            if re.match(r"^\.Lfunc_end\d+:$", line):
                raw.setdefault(name, []).append(("\n".join(body), desc))
                name = None
                continue
            tok = line.split()
            if tok[0] == ".amdhsa_kernel":
                in_desc = True
            elif tok[0] == ".end_amdhsa_kernel":
                in_desc = False
            elif in_desc:
                if tok[0] in DESC_FIELDS:
                    desc[tok[0]] = tok[1]
            elif tok[0] not in (".file", ".ident", ".section", ".p2align", ".text"):
                body.append(re.sub(r"\.L([A-Za-z]+)\d+_(\d+)", r".L\1_\2", line.strip()))
    pretty = demangle({n for name, vs in raw.items() for n in [name] + [m for t, _ in vs for m in MANGLED.findall(t)]})
    out = {}
    for name, vs in raw.items():
        vs = sorted((MANGLED.sub(lambda m: pretty[m.group(0)], t), sorted(d.items())) for t, d in vs)
        out[pretty[name]] = (vs, any(d for _, d in vs))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_tree")
    ap.add_argument("branch_tree")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly under DIR/parent and DIR/branch, reuse what is up to date")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    try:
        sides = [functions(assemble(os.path.abspath(t), os.path.join(tmp, sub))) for t, sub in ((a.parent_tree, "parent"), (a.branch_tree, "branch"))]
    finally:
        if not a.keep:
            shutil.rmtree(tmp, ignore_errors=True)
    parent, branch = sides
    bad = 0
    for name in sorted(set(parent) | set(branch)):
        if name not in branch or name not in parent:
            what = "only in the %s" % ("parent" if name in parent else "branch")
        elif parent[name] != branch[name]:
            (pv, _), (bv, _) = parent[name], branch[name]
            what = "descriptor differs" if [t for t, _ in pv] == [t for t, _ in bv] else "instructions differ"
        else:
            continue
        bad += 1
        print("DIFF  %s: %s" % (name, what))
    nk = sum(1 for _, k in branch.values() if k)
    print("isa_diff: %d of %d functions differ (%d kernels on the branch, %d on the parent)"
          % (bad, len(set(parent) | set(branch)), nk, sum(1 for _, k in parent.values() if k)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
