#!/usr/bin/env python3
"""Instruction census of the hot loop of rollout_cost_kernel<racing, fast, regen> from a hipcc -save-temps listing:
    python scripts/hot_loop.py /tmp/v/<name>/capi_solve-hip-amdgcn-amd-amdhsa-gfx950.s [--copy longest|unit_L|all] [--dump]
One iteration of a copy's loop = two racing steps + one float4 of noise.  The kernel holds one copy of the loop per
launch-uniform variant (mppi_rollout.hpp: lane_cost): a start outside the position clamp, the reference's unit wheel base
(ctx.unit_L, the copy the bench runs) and a general wheel base.  --copy longest (the default) is the longest
single-block loop (a general-wheel-base copy); --copy unit_L is the loop without the division by the wheel base: of the
copies that carry the full step (as many transcendentals as the longest), the one whose FMAs negate a single scalar
register — the map's cell size of Markstein's division, r = fma(-cell, q0, p) — where the general copies also negate the
wheel base, fma(-L, q0, vt).  The horizon is walked in two halves at two wave priorities (trajectory_cost, "Even drain"),
one copy of the loop each: both are reported, and it stops with an error unless there are one or two of them with the same
VALU and transcendental counts.  --copy all lists every copy."""
import collections
import re
import sys

KERNEL = "_ZN4mppi19rollout_cost_kernelILi4ELi2ELb1ELb1EEE"
TRANS = r"v_(log|sqrt|sin|cos|rcp|rsq|exp)_"


def loops(path):
    """Every single-block loop of the kernel: lists of instruction lines."""
    s = open(path).read()
    m = re.search(r"^(" + KERNEL + r"\w*):", s, re.M)
    body = s[m.start():s.index(".Lfunc_end", m.start())].split("\n")
    labels = {l.split(":")[0]: i for i, l in enumerate(body) if re.match(r"\.LBB\d+_\d+:", l)}
    out = []
    for i, l in enumerate(body):
        mm = re.match(r"\s+s_cbranch_\w+ (\.LBB\d+_\d+)", l)
        if mm and mm.group(1) in labels and labels[mm.group(1)] < i:
            j = labels[mm.group(1)]
            if not any(re.match(r"\.LBB", x) for x in body[j + 1:i]):
                out.append((mm.group(1), [x.strip() for x in body[j + 1:i + 1] if x.strip() and not x.strip().startswith(";")]))
    return out


def census(loop):
    ops = collections.Counter(l.split()[0] for l in loop)
    trans = sum(v for k, v in ops.items() if re.match(TRANS, k))
    valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    salu = sum(v for k, v in ops.items() if k.startswith("s_") and not k.startswith("s_waitcnt"))
    return ops, trans, valu, salu


def negated_sgprs(loop):
    """Scalar registers that the loop's FMAs take negated (v_fma_f32 vD, -sN, ...): the divisors of Markstein's sequences."""
    return {m for l in loop if l.startswith("v_fma") for m in re.findall(r"-(s\d+)\b", l)}


def report(label, loop):
    ops, trans, valu, salu = census(loop)
    print(f"[{label}] loop {len(loop)} instructions: VALU {valu} (transcendental {trans}, "
          f"v_mad_u64_u32 {ops.get('v_mad_u64_u32', 0)}, v_mad_u32_u24 {ops.get('v_mad_u32_u24', 0)}, "
          f"v_mov {ops.get('v_mov_b32_e32', 0)}), SALU {salu}, waitcnt {ops.get('s_waitcnt', 0)}, "
          f"LDS {sum(v for k, v in ops.items() if k.startswith('ds_'))}, "
          f"VMEM {sum(v for k, v in ops.items() if k.startswith(('global_', 'buffer_')))}")
    print("transcendental positions:", [i for i, l in enumerate(loop) if re.match(TRANS, l)])


def main():
    args = sys.argv[1:]
    copy = args[args.index("--copy") + 1] if "--copy" in args else "longest"
    all_loops = loops(args[0])
    if copy == "all":
        for label, loop in all_loops:
            report(label, loop)
        return
    longest = max(all_loops, key=lambda x: len(x[1]))
    if copy == "longest":
        label, loop = longest
    elif copy == "unit_L":
        full = [x for x in all_loops if census(x[1])[1] == census(longest[1])[1]]
        unit = [x for x in full if len(negated_sgprs(x[1])) == 1]
        if len(unit) not in (1, 2) or len({census(lp)[1:3] for _, lp in unit}) != 1:
            sys.exit(f"--copy unit_L: {len(unit)} full-step copies negate a single SGPR in their FMAs (expected 1, or the 2 "
                     "halves of the horizon with one VALU count): " + ", ".join(f"{lab} {sorted(negated_sgprs(lp))}" for lab, lp in full))
        for label, loop in unit[:-1]:
            report(label, loop)
        label, loop = unit[-1]
    else:
        sys.exit(f"unknown --copy {copy}")
    report(label, loop)
    if "--dump" in args:
        print("\n".join(loop))


if __name__ == "__main__":
    main()
