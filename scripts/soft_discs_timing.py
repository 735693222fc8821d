#!/usr/bin/env python3
"""What the graded skirt costs: the hard disc model against the soft one (reach 2, skirt 1) with n = 0, 1, 4, 8 discs, for
nav2d at N = 65 536, T = 50 and racing at N = 1 048 576, T = 50, fixed temperature, all in one session, the eight solvers of
a model taking turns (--rounds of them).

Per solver and round: the rollout stage from the stage timer (option "timing" = 2: the rollout stage only, stamped by the
kernel itself), drained after every solve; the median over the solves.  Reported per solver: median and spread (max - min)
over the rounds; per model and rule: the per-disc slope, a least-squares line through the medians at n = 0, 1, 4, 8.
Scenes, start states and the reference window are those of moving_discs_timing.py and racing_opponents_timing.py.
Usage: python scripts/soft_discs_timing.py [--model nav2d|racing|both] [--rounds 4] [--solves 40]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch

import mppi_playground_amd  # noqa: F401
from envs import MovingObstacleNav2DEnv, SoftMovingObstacleNav2DEnv
from envs.racing_opponents import (OpponentRacingEnv, SoftOpponentRacingEnv, opponent_racing_controller,
                                   soft_opponent_racing_controller)
from pi_mpc.mppi import MPPI

COUNTS = (0, 1, 4, 8)
SIZES = {"nav2d": (65536, 50), "racing": (1048576, 50)}


def build_nav2d(N, T, n, soft):
    env = (SoftMovingObstacleNav2DEnv if soft else MovingObstacleNav2DEnv)(horizon=T)
    k = np.arange(n, dtype=np.float32)
    pos = np.stack([-8.0 + 1.1 * k, -8.4 + 1.1 * k], 1) if n else np.zeros((0, 2), np.float32)
    vel = np.stack([0.3 * (-1.0) ** k, -0.4 * (-1.0) ** k], 1) if n else np.zeros((0, 2), np.float32)
    env.set_moving_obstacles(torch.from_numpy(pos), torch.from_numpy(vel.astype(np.float32)), 0.35)
    solver = MPPI(horizon=T, num_samples=N, dim_state=3, dim_control=2, dynamics=env.dynamics, cost_func=env.cost_function,
                  u_min=env.u_min, u_max=env.u_max, sigmas=torch.tensor([0.5, 0.5]), lambda_=5.0)
    assert solver._model == ("nav2d_discs_soft" if soft else "nav2d_discs")
    solver._keep = env
    return solver, env.reset().clone()


def build_racing(N, T, n, soft):
    env = (SoftOpponentRacingEnv if soft else OpponentRacingEnv)(horizon=T)
    env.set_opponents([30 + 25 * k for k in range(n)], [2.0 + 0.25 * k for k in range(n)], 0.9,
                      lateral_offset=[0.4 * (-1.0) ** k for k in range(n)])
    ctrl = (soft_opponent_racing_controller if soft else opponent_racing_controller)(env, horizon=T, num_samples=N, lambda_=1.0)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    x0 = env.reset().clone()
    ref, _ = ctrl.calc_ref_trajectory(x0, env.racing_center_path, 0, T, DL=0.1, lookahead_distance=3, reference_path_interval=0.85)
    ctrl.set_reference(ref)
    x0[3] = 4.0
    assert ctrl.solver._model == ("racing_discs_soft" if soft else "racing_discs")
    ctrl.solver._keep = ctrl
    return ctrl.solver, x0


def one_round(solver, x0, solves):
    for _ in range(5):
        solver.forward(x0)
    torch.cuda.synchronize()
    solver.set_option("timing", 2)
    solver.stage_times_ms()
    ro = []
    for _ in range(solves):
        solver.forward(x0)
        ro.append(solver.stage_times_ms()["rollout_cost"] * 1e3)
    solver.set_option("timing", 0)
    return statistics.median(ro)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="both", choices=("nav2d", "racing", "both"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--solves", type=int, default=40)
    args = ap.parse_args()
    for model in (("nav2d", "racing") if args.model == "both" else (args.model,)):
        N, T = SIZES[model]
        build = build_nav2d if model == "nav2d" else build_racing
        variants = [(rule, n) for n in COUNTS for rule in ("hard", "soft")]
        solvers = {v: build(N, T, v[1], v[0] == "soft") for v in variants}
        rows = {v: [] for v in variants}
        for _ in range(args.rounds):  # the solvers take turns inside every round
            for v in variants:
                rows[v].append(one_round(*solvers[v], args.solves))
        for rule in ("hard", "soft"):
            med = []
            for n in COUNTS:
                v = rows[rule, n]
                med.append(statistics.median(v))
                print(f"{model:6s} {rule} n={n} N={N} T={T} rollout stage " + "  ".join(f"{x:8.2f}" for x in v) +
                      f"  us   median {med[-1]:8.2f}  spread {max(v) - min(v):.2f}", flush=True)
            slope = np.polyfit(np.array(COUNTS, float), np.array(med), 1)[0]
            print(f"{model:6s} {rule} per-disc slope {slope:.2f} us (n = 1 over n = 0: {med[1] - med[0]:+.2f} us)", flush=True)
        solvers.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
