#!/usr/bin/env python
"""Kernel-by-kernel comparison of two source trees: registers, LDS, scratch, spills and instruction streams.

    python tools/kernel_resources.py --base ../parent-worktree [--out profiles/NAME.txt] [--jobs 8]

Compiles every entry of build.SOURCES of both trees (the tree this script lives in, and --base; each tree's own list, so a
source file may exist in one of them only) to gfx950 device assembly with build.py's flags (per-file EXTRA_FLAGS included)
plus `--offload-device-only -S`, then prints a two-column table: for every kernel symbol the metadata fields that decide
occupancy, the instruction count of its body, and whether the two instruction streams are the same text.  No GPU needed.
Exit status 1 when the symbol sets or any metadata field differ.
A stand-alone probe: nothing imports it.
"""
import argparse
import ast
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from dsml_thesis_amd import build  # noqa: E402  (flags and source list only)

FIELDS = (".vgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def tree_sources(root, only):
    """(SOURCES, EXTRA_FLAGS) as that tree's own build.py assigns them: a source file may exist in one tree only"""
    mod = ast.parse(open(os.path.join(root, "dsml_thesis_amd", "build.py")).read())
    lit = {n.targets[0].id: ast.literal_eval(n.value) for n in mod.body
           if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) in ("SOURCES", "EXTRA_FLAGS")}
    return [s for s in lit["SOURCES"] if not only or s in only], lit["EXTRA_FLAGS"]


def compile_tree(root, outdir, jobs, only):
    csrc = os.path.join(root, "dsml_thesis_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sources, extra = tree_sources(root, only)

    def one(src):
        out = os.path.join(outdir, src.replace(".hip", ".s"))
        cmd = [hipcc] + build.FLAGS + extra.get(src, []) + ["--offload-device-only", "-S", os.path.join(csrc, src), "-o", out]
        subprocess.check_call(cmd)
        return src, out

    with ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(one, sources))


def parse(path):
    """{kernel symbol: {field: int, 'insts': int, 'hash': str}} of one assembly file"""
    text = open(path).read()
    kernels = {}
    # metadata: one YAML record per kernel
    for rec in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""):
        name = re.search(r"\.name:\s+(\S+)", rec)
        if not name or ".symbol:" not in rec:
            continue
        kernels[name.group(1)] = {f: int(re.search(re.escape(f) + r":\s+(\d+)", rec).group(1)) for f in FIELDS}
    # bodies: from the symbol's label to its .Lfunc_end
    for sym, k in kernels.items():
        m = re.search(r"^" + re.escape(sym) + r":.*?^\.Lfunc_end\d+:", text, re.S | re.M)
        insts = []
        for line in m.group(0).split("\n")[1:]:
            line = line.split(";")[0].strip()
            if line and not line.startswith(".") and not line.endswith(":"):
                insts.append(re.sub(r"\s+", " ", line))
        k["insts"] = len(insts)
        k["hash"] = hashlib.sha256("\n".join(insts).encode()).hexdigest()
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", required=True, help="the tree to compare against (a worktree of the parent commit)")
    ap.add_argument("--out", help="also write the table here")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", help="comma-separated subset of build.SOURCES of either tree (default: all of them)")
    args = ap.parse_args()
    only = args.only.split(",") if args.only else None
    sides = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, root in (("base", os.path.abspath(args.base)), ("this", ROOT)):
            d = os.path.join(tmp, tag)
            os.makedirs(d)
            per_file = {}
            for src, path in compile_tree(root, d, args.jobs, only):
                for sym, k in parse(path).items():
                    per_file[(src, sym)] = k
            sides.append(per_file)
    base, this = sides
    lines = ["# base | this per kernel: " + " ".join(f[1:] for f in FIELDS) + " instructions; stream = same / DIFFERENT text",
             "# flags: " + " ".join(build.FLAGS) + " --offload-device-only -S (+ per-file EXTRA_FLAGS of build.py)"]
    bad = 0
    only_base, only_this = sorted(set(base) - set(this)), sorted(set(this) - set(base))
    for src, sym in only_base:
        lines.append(f"ONLY IN BASE {src} {sym}")
    for src, sym in only_this:
        lines.append(f"ONLY IN THIS {src} {sym}")
    bad += len(only_base) + len(only_this)
    n_same = n_diff = 0
    for key in sorted(set(base) & set(this)):
        b, t = base[key], this[key]
        meta_ok = all(b[f] == t[f] for f in FIELDS)
        same = b["hash"] == t["hash"]
        bad += 0 if meta_ok else 1
        n_same += same
        n_diff += not same
        cols = " ".join(f"{b[f]}|{t[f]}" for f in FIELDS)
        lines.append(f"{key[0]:20s} {cols} {b['insts']}|{t['insts']} {'same' if same else 'DIFFERENT'}{'' if meta_ok else ' METADATA-DIFFERS'} {key[1]}")
    lines.append(f"# {len(set(base) & set(this))} kernels in both trees, {len(only_base)} only in base, {len(only_this)} only in this; "
                 f"{n_same} identical instruction streams, {n_diff} different; metadata mismatches: {bad - len(only_base) - len(only_this)}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        notes = ""          # a leading block of "## " lines (hand-written findings) in an existing --out file survives the re-run
        if os.path.exists(args.out):
            for line in open(args.out):
                if not line.startswith("## "):
                    break
                notes += line
        with open(args.out, "w") as fh:
            fh.write(notes + text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
