#!/usr/bin/env python3
"""Say, kernel by kernel, whether two builds of the device code have the same gfx950 instruction text.

    python tools/kernel_text_diff.py OLD NEW [--filter baked] [--jobs N]

OLD and NEW are each a source tree (every pixel-nerf_amd/csrc/pnr_*.hip of it is compiled, or only those whose name holds
--filter), a single .hip file, a single .s file, or a directory of .s files.  Sources are compiled device-side only to assembly
with the library's flags (hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S); nothing needs a GPU.

A kernel's text is the instructions between its label and its .Lfunc_end, comments and directives dropped and the block labels
(.LBBn_m) renumbered in order of first appearance, so a kernel that merely moved within its unit, or to another unit, compares
equal.  Kernels are matched by demangled name across ALL units of a side: a refactor that moves a kernel to another file shows
it as `same`.  Prints one line per kernel -- same / DIFFERENT / only in OLD / only in NEW -- with the instruction counts, then
the totals.  Exit status 0 whatever the result: the tool compares and counts, the reader judges."""
import argparse
import glob
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Wno-unused-value"]


def compile_to_s(src, outdir):
    out = os.path.join(outdir, os.path.basename(src)[:-4] + ".s")
    subprocess.run([shutil.which("hipcc") or "/opt/rocm/bin/hipcc", *FLAGS, src, "-o", out], check=True)
    return out


def assembly_files(path, flt, outdir, jobs):
    if os.path.isfile(path):
        srcs = [path]
    elif glob.glob(os.path.join(path, "*.s")):
        srcs = sorted(glob.glob(os.path.join(path, "*.s")))
    else:
        srcs = sorted(glob.glob(os.path.join(path, "pixel-nerf_amd", "csrc", "pnr_*.hip")))
    srcs = [s for s in srcs if not flt or flt in os.path.basename(s)]
    if not srcs:
        raise SystemExit(f"{path}: nothing to compare")
    os.makedirs(outdir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=jobs) as pool:
        return list(pool.map(lambda s: s if s.endswith(".s") else compile_to_s(s, outdir), srcs))


def kernels(s_file):
    """{mangled kernel name: [instruction lines, labels renumbered]} of one assembly file"""
    lines = open(s_file).read().splitlines()
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    out, cur, labels = {}, None, {}
    for raw in lines:
        line = raw.split(";")[0].rstrip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m and m.group(1) in names:
            cur, labels = m.group(1), {}
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        text = line.strip()
        if not text or (text.startswith(".") and not text.startswith(".LBB")):
            continue  # a directive
        text = re.sub(r"\.LBB\d+_\d+", lambda k: labels.setdefault(k.group(0), f".L{len(labels)}"), text)
        out[cur].append(re.sub(r"\s+", " ", text))
    return out


def side(path, flt, outdir, jobs):
    found = {}
    for f in assembly_files(path, flt, outdir, jobs):
        found.update(kernels(f))
    mangled = list(found)
    plain = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"^void ", "", p.strip()): found[m] for m, p in zip(mangled, plain)}


def count(text):
    return sum(1 for t in text if not t.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--filter", default=None, help="only the units whose file name holds this")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        old = side(a.old, a.filter, os.path.join(td, "old"), a.jobs)
        new = side(a.new, a.filter, os.path.join(td, "new"), a.jobs)
    tally = {"same": 0, "DIFFERENT": 0, "only in OLD": 0, "only in NEW": 0}
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        what = "only in NEW" if o is None else "only in OLD" if n is None else "same" if o == n else "DIFFERENT"
        tally[what] += 1
        short = re.sub(r"\(.*\)$", "", name)
        print(f"{what:11s} {count(o) if o is not None else '-':>6} {count(n) if n is not None else '-':>6}  {short}")
    print("; ".join(f"{v} {k}" for k, v in tally.items()) +
          f"; instructions {sum(map(count, old.values()))} -> {sum(map(count, new.values()))}")


if __name__ == "__main__":
    main()
