#!/usr/bin/env python3
"""What a risk-aware solve costs: racing with P = 1, 2, 4, 8, 16 state particles against the plain solve, at the example's
size (N = 4 000, T = 25) and at N = 1 048 576, T = 50 (P = 4), fixed temperature, all in one session, the solvers of a size
taking turns (--rounds of them).

Per solver and round: the solve from the host clock (a batch of --solves forward() calls, synchronised once, timing off) and
the rollout stage from the stage timer (option "timing" = 2, "timing_source" = 1: event pairs on the stage's dispatches for
every solver, so that the plain kernel's in-kernel stamps and the particle stage's two dispatches are measured alike), drained
after every solve; the median over the solves.  Reported per solver: median and spread (max - min) over the rounds.  The
fold's own time at the large size: mppi_set_particle_costs from a device matrix (copy + fold) minus the same copy alone, from
event pairs.  A tree without set_state_particles (the parent commit) runs the plain solvers only.
Usage: python scripts/particles_timing.py [--size small|large|both] [--rounds 4] [--solves 30]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch

import mppi_playground_amd  # noqa: F401
from envs.racing_controller import racing_controller
from envs.racing_env import RacingEnv

SIZES = {"small": (4000, 25, (1, 2, 4, 8, 16)), "large": (1048576, 50, (4,))}


def build(N, T, P, fused=True):
    env = RacingEnv()
    ctrl = racing_controller(env, horizon=T, num_samples=N, lambda_=1.0)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    x0 = env.reset().clone()
    ref, _ = ctrl.calc_ref_trajectory(x0, env.racing_center_path, 0, T, DL=0.1, lookahead_distance=3, reference_path_interval=0.85)
    ctrl.set_reference(ref)
    x0[3] = 4.0
    solver = ctrl.solver
    solver._keep = ctrl
    if not fused:
        solver.set_option("fused_solve", 0)
    if P:
        rng = np.random.default_rng(P)
        parts = x0.cpu().numpy()[None, :] + rng.normal(0.0, 1.0, (P, 4)).astype(np.float32) * np.float32([0.2, 0.2, 0.05, 0.3])
        solver.set_state_particles(torch.from_numpy(parts.astype(np.float32)).cuda())
    return solver, x0


def one_round(solver, x0, solves):
    for _ in range(5):
        solver.forward(x0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(solves):
        solver.forward(x0)
    torch.cuda.synchronize()
    solve_us = (time.perf_counter() - t0) / solves * 1e6
    solver.set_option("timing_source", 1)
    solver.set_option("timing", 2)
    solver.stage_times_ms()
    ro = []
    for _ in range(solves):
        solver.forward(x0)
        ro.append(solver.stage_times_ms()["rollout_cost"] * 1e3)
    solver.set_option("timing", 0)
    return solve_us, statistics.median(ro)


def fold_alone(solver, P, N, reps=20):
    """us: (copy + fold) - copy, medians of event pairs"""
    src = solver.particle_costs.clone()
    dst = torch.empty_like(src)
    st = solver._stream()
    both, copy = [], []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        solver._h.call("mppi_set_particle_costs", src.data_ptr(), 1, st)
        e[1].record()
        e[2].record()
        dst.copy_(src)
        e[3].record()
        torch.cuda.synchronize()
        both.append(e[0].elapsed_time(e[1]) * 1e3)
        copy.append(e[2].elapsed_time(e[3]) * 1e3)
    return statistics.median(both), statistics.median(copy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="both", choices=("small", "large", "both"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--solves", type=int, default=30)
    args = ap.parse_args()
    from pi_mpc.mppi import MPPI

    have = hasattr(MPPI, "set_state_particles")
    for size in (("small", "large") if args.size == "both" else (args.size,)):
        N, T, counts = SIZES[size]
        variants = [("plain", 0, True), ("plain multi-kernel", 0, False)] + ([(f"P={P}", P, True) for P in counts] if have else [])
        solvers = {v[0]: build(N, T, v[1], v[2]) for v in variants}
        rows = {v[0]: [] for v in variants}
        for _ in range(args.rounds):  # the solvers take turns inside every round
            for name in rows:
                rows[name].append(one_round(*solvers[name], args.solves))
        for name, v in rows.items():
            for what, col in (("solve", 0), ("rollout stage", 1)):
                x = [r[col] for r in v]
                print(f"racing N={N} T={T} {name:18s} {what:13s} " + "  ".join(f"{t:9.2f}" for t in x) +
                      f"  us   median {statistics.median(x):9.2f}  spread {max(x) - min(x):.2f}", flush=True)
        if have and size == "large":
            P = counts[0]
            both, copy = fold_alone(solvers[f"P={P}"][0], P, N)
            print(f"racing N={N} P={P} fold alone: copy + fold {both:.2f} us, copy {copy:.2f} us, fold {both - copy:.2f} us", flush=True)
        solvers.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
