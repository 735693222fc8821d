#!/usr/bin/env python3
"""Device-assembly gate for changes that must not move a kernel: compiles every unit of the library to gfx950 assembly from
the working tree and from <parent-rev> and compares them kernel by kernel.

Both trees are compiled with _build.FLAGS minus -shared / -fPIC, plus --cuda-device-only -S; <parent-rev>'s csrc/ and
include/ are checked out into a temporary directory.  Lines that name the per-unit `__hip_cuid_<hash>` symbol are dropped
(the hash follows the source text), and the ordinal of a function inside its unit is taken out of its local labels, so a
new template instantiation does not show up as a change of every kernel behind it.  Per unit the script prints
`identical`, or the mangled names of the kernels whose text differs (new ones: `only in the tree`).  Nothing else about the assembly is printed.  Exit status 1 unless every unit is identical.

Usage: python scripts/device_asm_diff.py <parent-rev> [--jobs N]   (N <= 16, default 8; needs hipcc, no GPU)"""
import argparse
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mppi_playground_amd import _build  # noqa: E402

CSRC_REL = os.path.relpath(_build.CSRC, ROOT)
FLAGS = [f for f in _build.FLAGS if f not in ("-shared", "-fPIC")] + ["--cuda-device-only", "-S"]


def compile_unit(csrc, src, out):
    r = subprocess.run([_build.hipcc(), *FLAGS, "-o", out, src], cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f"{src} in {csrc}:\n{r.stderr[-2000:]}")
    return out


def functions(path):
    """{symbol: text} of the listing's functions (from the .type ...,@function line to .Lfunc_end) and kernel descriptors
    (.amdhsa_kernel to .end_amdhsa_kernel), plus what lies outside all of them under the key None."""
    out, rest, name, cur = {}, [], None, None
    with open(path) as f:
        for ln in f:
            if "__hip_cuid_" in ln:
                continue
            # local labels carry the function's ordinal in its unit (.LBB<k>_<n>, .Lfunc_begin<k>, .Lfunc_end<k>, .LJTI<k>_<n>,
            # and BB<k>_<n> in the loop comments): a new template instantiation ahead of a kernel renumbers them without touching
            # an instruction (and moves the column of the comment behind a label by a digit)
            ln = re.sub(r"\.(LBB|LJTI|Lfunc_begin|Lfunc_end)\d+", r".\1#", ln)
            ln = re.sub(r"\s+;", " ;", re.sub(r"\bBB\d+_", "BB#_", ln))
            m = re.match(r"\s*\.type\s+([^,\s]+),@function", ln) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
            if m:
                if cur is not None:  # (a kernel's descriptor follows its code, before .Lfunc_end)
                    out[name] = "".join(cur)
                name, cur = m.group(1) + (" (kernel descriptor)" if ".amdhsa_kernel" in ln else ""), []
            if cur is None:
                rest.append(ln)
                continue
            cur.append(ln)
            if ln.startswith(".Lfunc_end") or ".end_amdhsa_kernel" in ln:
                out[name] = "".join(cur)
                name, cur = None, None
    out[None] = "".join(rest)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    jobs = max(1, min(a.jobs, 16))
    with tempfile.TemporaryDirectory() as tmp:
        tar = os.path.join(tmp, "parent.tar")
        subprocess.check_call(["git", "archive", "-o", tar, a.parent, CSRC_REL, "include"], cwd=ROOT)
        with tarfile.open(tar) as t:
            t.extractall(os.path.join(tmp, "parent"))
        trees = {"parent": os.path.join(tmp, "parent", CSRC_REL), "tree": _build.CSRC}
        parent_sources = [s for s in _build.SOURCES if os.path.exists(os.path.join(trees["parent"], s))]
        with ThreadPoolExecutor(jobs) as ex:  # (the big units first: they decide the wall time)
            order = sorted(_build.SOURCES, key=lambda s: -os.path.getsize(os.path.join(_build.CSRC, s)))
            fut = {(k, s): ex.submit(compile_unit, trees[k], s, os.path.join(tmp, f"{k}_{s}.s"))
                   for s in order for k in trees if k == "tree" or s in parent_sources}
            listing = {key: f.result() for key, f in fut.items()}
        bad = 0
        for s in _build.SOURCES:
            if s not in parent_sources:
                print(f"{s}: not in {a.parent}")
                bad += 1
                continue
            p, n = functions(listing["parent", s]), functions(listing["tree", s])
            differ = sorted(k for k in set(p) | set(n) if k is not None and p.get(k) != n.get(k))
            if not differ and p[None] == n[None] and list(p) == list(n):
                print(f"{s}: identical ({sum(1 for k in p if k and k.endswith('(kernel descriptor)'))} kernels)")
                continue
            bad += 1
            print(f"{s}: DIFFERS")
            for k in differ:
                print(f"    {k}" + ("" if k in p and k in n else "  (only in the parent)" if k in p else "  (only in the tree)"))
            if not differ:
                print("    (no function's text: their order, or the text outside the functions)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
