#!/usr/bin/env python3
"""Instruction census of EVERY loop of one kernel in a hipcc `-S` (or -save-temps) listing, nested loops included:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fhip-fp32-correctly-rounded-divide-sqrt \\
          --cuda-device-only -S -o solve.s mppi_playground_amd/csrc/capi_solve.hip
    python scripts/loop_census.py solve.s [mangled kernel name prefix]
scripts/hot_loop.py reads the racing kernel's single-block loops only; a kernel whose horizon loop holds another loop (the
moving-disc model: the loop over the discs of a row, default kernel here) is not a single block.  Per backward branch: the
label, the line range, the basic blocks inside, instructions, VALU, LDS reads and transcendentals between the label and the
branch.  An outer loop's figures INCLUDE its inner loops' bodies once: subtract them for the loop's own instructions."""
import re
import sys

KERNEL = "_ZN4mppi19rollout_cost_kernelILi9ELi2ELb1ELb1EEE"  # rollout_cost_kernel<NAV2D_DISCS, 2, true, true>
TRANS = r"v_(log|sqrt|sin|cos|rcp|rsq|exp)_"


def main():
    s = open(sys.argv[1]).read()
    name = sys.argv[2] if len(sys.argv) > 2 else KERNEL
    m = re.search(r"^(" + re.escape(name) + r"\w*):", s, re.M)
    if not m:
        sys.exit(f"no kernel {name} in the listing")
    body = s[m.start():s.index(".Lfunc_end", m.start())].split("\n")
    labels = {l.split(":")[0]: i for i, l in enumerate(body) if re.match(r"\.LBB\d+_\d+:", l)}
    print(f"{m.group(1)}: {len(body)} lines")
    print("loop         lines        blocks instr  VALU  ds_read trans")
    for i, l in enumerate(body):
        mm = re.match(r"\s+s_c?branch\w* (\.LBB\d+_\d+)", l)
        if not (mm and mm.group(1) in labels and labels[mm.group(1)] < i):
            continue
        j = labels[mm.group(1)]
        ins = [x.strip() for x in body[j + 1:i + 1]
               if x.strip() and not x.strip().startswith(";") and not re.match(r"\.LBB", x.strip())]
        inner = sum(1 for x in body[j + 1:i] if re.match(r"\.LBB", x))
        print(f"{mm.group(1):12s} {j:5d}-{i:<5d} {inner:6d} {len(ins):5d} {sum(x.startswith('v_') for x in ins):5d} "
              f"{sum(x.startswith('ds_read') for x in ins):8d} {sum(bool(re.match(TRANS, x)) for x in ins):5d}")


if __name__ == "__main__":
    main()
