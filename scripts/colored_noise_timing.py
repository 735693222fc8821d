#!/usr/bin/env python3
"""Price of temporally correlated sampling noise (MPPI(..., noise_beta=...)) at the headline size (racing, N = 2^20, T = 50,
lambda = 1): the `sample` stage and the whole solve of a colored solver against the unfiltered solver at noise_regen = 0 (the
same materialised-noise path with sample_kernel as the draw), and the default regenerating solve for context.

Per figure: the median over 60 solves after 20 warm-up solves, three repetitions.  Stage times come from mppi_get_timing
(option "timing" = 1, drained after every solve, so every solve contributes one value per stage); `stages` is their sum, the
solve's device time.  `open loop` is wall clock per solve over 60 back-to-back solves with timing off (one figure per
repetition, no median inside it).
Usage: python scripts/colored_noise_timing.py [--beta 0.9] [--samples 1048576]"""
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

T = 50
STAGES = ("sample", "rollout_cost", "weights_reduce", "finalize")


def build(N, **kw):
    env = RacingEnv()
    ctrl = racing_controller(env, horizon=T, num_samples=N, lambda_=1.0, **kw)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    ref, _ = ctrl.calc_ref_trajectory(env._robot_state, env.racing_center_path, 0, T, DL=0.1, lookahead_distance=3,
                                      reference_path_interval=0.85)
    ctrl.set_reference(ref)
    ctrl.solver._keep = ctrl
    return ctrl.solver, env._robot_state.clone().cuda()


def loop(solver, x0, n):
    for _ in range(n):
        solver.forward(x0)
    torch.cuda.synchronize()


def measure(solver, x0, n=60, warm=20):
    """(median of every stage, median sum of the stages, open-loop wall clock), all in us per solve."""
    loop(solver, x0, warm)
    solver.set_option("timing", 1)
    solver.stage_times_ms()
    per, stages = {s: [] for s in STAGES}, []
    for _ in range(n):
        solver.forward(x0)
        t = solver.stage_times_ms()
        for s in STAGES:
            per[s].append(t[s] * 1e3)
        stages.append(sum(t[s] for s in STAGES) * 1e3)
    solver.set_option("timing", 0)
    loop(solver, x0, warm)
    t0 = time.perf_counter()
    loop(solver, x0, n)
    wall = (time.perf_counter() - t0) / n * 1e6
    return [statistics.median(per[s]) for s in STAGES] + [statistics.median(stages), wall]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beta", type=float, default=0.9)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    # (the third case draws the unfiltered noise through the per-column sigma table, sample_kernel<true>: its `sample` stage is
    # the table-reading sampler's; its other stages carry the adaptation's own launches and are not a comparator)
    # (beta = 0.001 runs the colored path on noise that is the unfiltered noise to three digits: what the PATH costs, apart
    # from what smoother samples do to the rollout's map lookups and to the number of tiles that carry weight)
    cases = (("colored", dict(noise_beta=args.beta), None), ("colored, beta = 0.001", dict(noise_beta=1e-3), None),
             ("unfiltered, noise_regen = 0", {}, 0),
             ("unfiltered, sigma table", dict(adapt_covariance=True, cov_rate=0.0), None), ("default (regenerating)", {}, 1))
    for name, kw, regen in cases:
        solver, x0 = build(args.samples, **kw)
        if regen is not None:
            solver.set_option("noise_regen", regen)
        rows = [measure(solver, x0) for _ in range(args.reps)]
        for col, what in enumerate(STAGES + ("stages", "open loop")):
            vals = [r[col] for r in rows]
            print(f"{name:28s} {what:15s} " + "  ".join(f"{v:8.2f}" for v in vals) + f"  us   (spread {max(vals) - min(vals):.2f})", flush=True)
        del solver


if __name__ == "__main__":
    main()
