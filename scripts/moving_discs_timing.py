#!/usr/bin/env python3
"""What the moving-disc model costs: plain nav2d against nav2d_discs with n = 0, 1, 4, 8 discs at the size of configuration C2
(N = 65 536, T = 50) and a fixed temperature, all in one session, the five solvers taking turns (--rounds of them).

Per solver and round: the open-loop wall clock per solve (timing off) and the rollout stage from mppi_get_timing (option
"timing" = 1, drained after every solve; the median over the solves).  Reported: median and spread (max - min) over the rounds.
Then the per-tick cost of handing over a new table (mppi_set_discs), from a host table and from a device table: host time of
the call (it does not wait) and the wall clock of call + stream synchronisation.
Usage: python scripts/moving_discs_timing.py [--size 65536x50] [--rounds 4] [--solves 60]"""
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
from envs import MovingObstacleNav2DEnv
from envs.navigation_2d import Navigation2DEnv
from pi_mpc.mppi import MPPI

LAMBDA = 5.0


def discs(env, n):
    """n discs spread along the start-goal diagonal, drifting across it: some are met inside the horizon, most are not"""
    k = np.arange(n, dtype=np.float32)
    pos = np.stack([-8.0 + 1.1 * k, -8.4 + 1.1 * k], 1) if n else np.zeros((0, 2), np.float32)
    vel = np.stack([0.3 * (-1.0) ** k, -0.4 * (-1.0) ** k], 1) if n else np.zeros((0, 2), np.float32)
    env.set_moving_obstacles(torch.from_numpy(pos), torch.from_numpy(vel.astype(np.float32)), 0.35)


def build(N, T, n):
    if n is None:
        env = Navigation2DEnv()
    else:
        env = MovingObstacleNav2DEnv(horizon=T)
        discs(env, n)
    solver = MPPI(horizon=T, num_samples=N, dim_state=3, dim_control=2, dynamics=env.dynamics, cost_func=env.cost_function,
                  u_min=env.u_min, u_max=env.u_max, sigmas=torch.tensor([0.5, 0.5]), lambda_=LAMBDA)
    assert solver._model == ("nav2d" if n is None else "nav2d_discs")
    solver._keep = env
    return solver, env.reset().clone()


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


def handover(solver, T, on_device, reps=200):
    tab = np.zeros((T, 8, 4), np.float32)
    tab[:, :, 2], tab[:, :, 3] = 0.1, 10.0
    dev = torch.from_numpy(tab).cuda()
    st = solver._stream()
    call = (lambda: solver._h.call("mppi_set_discs", dev.data_ptr(), T, 8, 1, st)) if on_device else \
           (lambda: solver._h.call("mppi_set_discs", tab.ctypes.data_as(C.c_void_p), T, 8, 0, st))
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    host, total = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append((t1 - t0) * 1e6)
        total.append((t2 - t0) * 1e6)
    return statistics.median(host), statistics.median(total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="65536x50")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--solves", type=int, default=60)
    args = ap.parse_args()
    N, T = (int(v) for v in args.size.split("x"))
    variants = [("nav2d", None), ("discs n=0", 0), ("discs n=1", 1), ("discs n=4", 4), ("discs n=8", 8)]
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
    s8 = solvers["discs n=8"][0]
    for on_device in (False, True):
        h, t = handover(s8, T, on_device)
        print(f"mppi_set_discs rows={T} n=8 from a {'device' if on_device else 'host'} table: call {h:.2f} us, call + sync {t:.2f} us", flush=True)


if __name__ == "__main__":
    main()
