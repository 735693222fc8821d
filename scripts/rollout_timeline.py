#!/usr/bin/env python3
"""Per-SIMD timeline of one rollout launch of the metric's workload (racing, lambda = 1) from a -DMPPI_ROLLOUT_TRACE build:
    python scripts/rollout_timeline.py [--name trace] [--flags=-DMPPI_AB_NO_DRAIN_PRIO] [--samples N] [--horizon T] [--launches K]
builds mppi_playground_amd/csrc/variants/lib_<name>.so with scripts/build_variant.sh unless it is there already, then runs
itself in a child process that loads it (MPPI_HIP_LIB).  Lane 0 of every wave stamps the 100 MHz clock at its entry, behind the
prologue's barrier, at the entry and the exit of the horizon loop and at the end of its block, and stores HW_REG_HW_ID and
HW_REG_XCC_ID (csrc/mppi_rollout.hpp).  Reported per launch, as median [min .. max] over the SIMDs that ran a wave:
  waves per SIMD; when the waves of a SIMD left the loop, counted back from the SIMD's last one; how long the SIMD held fewer
  than two waves still inside their loops before its last wave left ("under-filled drain"); the last wave's time per group
  of the horizon loop against the waves that entered the loop in the first fifth of the launch; and over the waves, the
  prologue (entry -> loop entry, with its part up to the barrier) of the first-dispatched round and of the later ones."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICK_US = 0.01  # the wall clock runs at 100 MHz


def stats(x):
    import numpy as np

    x = np.asarray(x, np.float64)
    return f"{np.median(x):.2f} [{x.min():.2f} .. {x.max():.2f}]" if x.size else "-"


def analyse(rows, groups):
    """rows: int64 [waves][6] of one launch (waves that did not run are all zero)."""
    import numpy as np

    rows = rows[rows[:, 0] != 0].copy()
    # column 2 holds the low words of the loop's two stamps (entry | exit << 32): rebuilt from the barrier stamp in front of them
    for col, word in ((3, (rows[:, 2] >> 32) & 0xFFFFFFFF), (2, rows[:, 2] & 0xFFFFFFFF)):
        rows[:, col] = rows[:, 1] + ((word - (rows[:, 1] & 0xFFFFFFFF)) & 0xFFFFFFFF)
    t = (rows[:, :5] - rows[:, 0].min()) * TICK_US  # us since the first wave's entry
    hw, xcc = rows[:, 5] & 0xFFFFFFFF, (rows[:, 5] >> 32) & 0xF
    simd = (xcc << 16) | (hw & 0xFF30)  # XCC_ID; HW_ID: SE_ID [15:13], SH_ID [12], CU_ID [11:8], SIMD_ID [5:4]
    keys = np.unique(simd)
    span = t[:, 4].max()
    first_round = t[:, 0] < 0.05 * span  # (a later wave starts when an earlier one ends: far beyond this)
    early = t[:, 2] < 0.2 * span
    per_group = (t[:, 3] - t[:, 2]) / max(groups, 1)
    counts, back, under, last_rate, last_end = [], [[] for _ in range(3)], [], [], []
    for k in keys:
        m = simd == k
        enter, leave = t[m, 2], np.sort(t[m, 3])
        counts.append(int(m.sum()))
        last_end.append(leave[-1])
        for j in range(3):
            if leave.size > j + 1:
                back[j].append(leave[-1] - leave[-2 - j])
        # once the SIMD's last wave has entered its loop no more work arrives: from there to the last exit, the time during
        # which fewer than two waves were still inside their loops
        ev = sorted([(x, 1) for x in enter] + [(x, -1) for x in leave])
        inside, prev, lack = 0, 0.0, 0.0
        for x, dlt in ev:
            if prev >= enter.max() and inside < 2:
                lack += x - prev
            inside += dlt
            prev = x
        under.append(lack)
        last_rate.append(per_group[m][np.argmax(t[m, 3])])
    print(f"  waves {rows.shape[0]} on {keys.size} SIMDs, {stats(counts)} per SIMD; first entry -> last block end {span:.2f} us; "
          f"last loop exit of a SIMD at {stats(last_end)} us")
    print("  loop exits counted back from the SIMD's last: " + ", ".join(f"{j + 2}. last -{stats(b)}" for j, b in enumerate(back)) + " us")
    print(f"  under-filled drain (fewer than two waves in their loops, before the last exit): {stats(under)} us")
    print(f"  us per group of the horizon loop: last wave of a SIMD {stats(last_rate)}, waves that entered in the first fifth "
          f"{stats(per_group[early])}, all {stats(per_group)}")
    for label, m in (("first-dispatched round", first_round), ("later rounds", ~first_round)):
        print(f"  prologue, {label} ({int(m.sum())} waves): entry -> loop entry {stats((t[:, 2] - t[:, 0])[m])} us, of which "
              f"entry -> barrier {stats((t[:, 1] - t[:, 0])[m])} us")
    print(f"  loop exit -> block end {stats(t[:, 4] - t[:, 3])} us", flush=True)


def child(args):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch

    import mppi_playground_amd  # noqa: F401
    from envs.racing_controller import racing_controller
    from envs.racing_env import RacingEnv

    env = RacingEnv()
    x0 = env.reset().clone()
    T, N = args.horizon, args.samples
    ctrl = racing_controller(env, horizon=T, num_samples=N, lambda_=1.0)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    ref, _ = ctrl.calc_ref_trajectory(x0, env.racing_center_path, 0, T, DL=0.1, lookahead_distance=3, reference_path_interval=0.85)
    ctrl.set_reference(ref)
    solver, x0 = ctrl.solver, x0.cuda()
    arm = solver._h.lib.mppi_debug_rollout_trace
    arm.argtypes, arm.restype = [C.c_void_p], C.c_int
    blocks = ((N + 63) // 64 + 3) // 4 + 1
    rows = torch.zeros((4 * blocks, 6), dtype=torch.int64, device="cuda")
    for _ in range(args.warmup):
        solver.forward(x0)
    torch.cuda.synchronize()
    print(f"{os.path.basename(os.environ['MPPI_HIP_LIB'])}: racing N = {N}, T = {T} ({T // 2} groups)")
    for k in range(args.launches):
        rows.zero_()
        torch.cuda.synchronize()
        assert arm(rows.data_ptr()) == 0
        solver.forward(x0)
        torch.cuda.synchronize()
        assert arm(None) == 0
        print(f" launch {k}:")
        analyse(rows.cpu().numpy(), T // 2)
        for _ in range(5):
            solver.forward(x0)
    if args.out:
        np.save(args.out, rows.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="trace")
    ap.add_argument("--flags", default="", help="further hipcc flags of the variant, space separated")
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default="", help="save the last launch's rows (.npy)")
    args = ap.parse_args()
    if os.environ.get("MPPI_ROLLOUT_TIMELINE_CHILD"):
        return child(args)
    lib = os.path.join(ROOT, "mppi_playground_amd", "csrc", "variants", f"lib_{args.name}.so")
    if not os.path.exists(lib):
        subprocess.check_call([os.path.join(ROOT, "scripts", "build_variant.sh"), args.name, "-DMPPI_ROLLOUT_TRACE", *args.flags.split()])
    env = dict(os.environ, MPPI_HIP_LIB=lib, MPPI_ROLLOUT_TIMELINE_CHILD="1")
    return subprocess.call([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env)


if __name__ == "__main__":
    sys.exit(main())
