#!/usr/bin/env python3
"""What racing among opponent cars costs: plain racing against racing_discs with n = 0, 1, 4, 8 cars at the flagship size
(N = 1 048 576, T = 50) or the example's (--size 4000x25), fixed temperature, all in one session, the five solvers taking turns
(--rounds of them).

Per solver and round: the open-loop wall clock per solve (timing off) and the rollout stage from mppi_get_timing (option
"timing" = 1, drained after every solve; the median over the solves).  Reported: median and spread (max - min) over the rounds.
The reference window is the example's from the start pose (uploaded once), the start state the start pose at 4 m/s.
Usage: python scripts/racing_opponents_timing.py [--size 1048576x50] [--rounds 4] [--solves 40]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch

import mppi_playground_amd  # noqa: F401
from envs.racing_controller import racing_controller
from envs.racing_env import RacingEnv
from envs.racing_opponents import OpponentRacingEnv, opponent_racing_controller

LAMBDA = 1.0


def build(N, T, n):
    if n is None:
        env = RacingEnv()
        ctrl = racing_controller(env, horizon=T, num_samples=N, lambda_=LAMBDA)
    else:
        env = OpponentRacingEnv(horizon=T)
        # n cars ahead on alternating sides of the centre line: the first ones are met inside the horizon
        env.set_opponents([30 + 25 * k for k in range(n)], [2.0 + 0.25 * k for k in range(n)], 0.9,
                          lateral_offset=[0.4 * (-1.0) ** k for k in range(n)])
        ctrl = opponent_racing_controller(env, horizon=T, num_samples=N, lambda_=LAMBDA)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    x0 = env.reset().clone()
    ref, _ = ctrl.calc_ref_trajectory(x0, env.racing_center_path, 0, T, DL=0.1, lookahead_distance=3, reference_path_interval=0.85)
    ctrl.set_reference(ref)
    x0[3] = 4.0
    assert ctrl.solver._model == ("racing" if n is None else "racing_discs")
    ctrl.solver._keep = ctrl
    return ctrl.solver, x0


def loop(solver, x0, n):
    for _ in range(n):
        solver.forward(x0)
    torch.cuda.synchronize()


def one_round(solver, x0, solves):
    loop(solver, x0, 10)
    t0 = time.perf_counter()
    loop(solver, x0, solves)
    wall = (time.perf_counter() - t0) / solves * 1e6
    solver.set_option("timing", 1)
    solver.stage_times_ms()
    ro = []
    for _ in range(solves):
        solver.forward(x0)
        ro.append(solver.stage_times_ms()["rollout_cost"] * 1e3)
    solver.set_option("timing", 0)
    return wall, statistics.median(ro)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1048576x50")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--solves", type=int, default=40)
    args = ap.parse_args()
    N, T = (int(v) for v in args.size.split("x"))
    variants = [("racing", None), ("discs n=0", 0), ("discs n=1", 1), ("discs n=4", 4), ("discs n=8", 8)]
    solvers = {name: build(N, T, n) for name, n in variants}
    rows = {name: [] for name, _ in variants}
    for _ in range(args.rounds):  # the solvers take turns inside every round
        for name, _ in variants:
            rows[name].append(one_round(*solvers[name], args.solves))
    for name, _ in variants:
        for col, what in enumerate(("open loop", "rollout stage")):
            v = [r[col] for r in rows[name]]
            print(f"{name:10s} N={N} T={T} {what:13s} " + "  ".join(f"{x:8.2f}" for x in v) +
                  f"  us   median {statistics.median(v):8.2f}  spread {max(v) - min(v):.2f}", flush=True)


if __name__ == "__main__":
    main()
