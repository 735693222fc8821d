#!/usr/bin/env python3
"""Price of the opt-in control-cost term (MPPI(..., action_cost=True)): C3 (racing N = 2^20, T = 50, lambda = 1) and C2 (nav2d
N = 65 536, T = 50, lambda = 1), term on against off in one session, best of three 50-solve open loops after 20 warm-up
solves, us per solve and the rollout stage's own time; plus the comparator the fused placement avoids — a separate pass that
has to materialise the noise first: sample_kernel's time (noise_regen = 0) and mppi_add_action_cost's own.
Usage: python scripts/action_cost_timing.py [c3|c2|both] [--loop-only]   (--loop-only: one on / off loop each, for profilers)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch

import mppi_playground_amd  # noqa: F401
from envs.navigation_2d import Navigation2DEnv
from envs.racing_controller import racing_controller
from envs.racing_env import RacingEnv

T = 50


def build(which, **kw):
    if which == "c3":
        env = RacingEnv()
        ctrl = racing_controller(env, horizon=T, num_samples=1 << 20, lambda_=1.0, **kw)
        ctrl.set_cost_map(env._obstacle_map, env._lane_map)
        ref, _ = ctrl.calc_ref_trajectory(env._robot_state, env.racing_center_path, 0, T, DL=0.1, lookahead_distance=3,
                                          reference_path_interval=0.85)
        ctrl.set_reference(ref)
        ctrl.solver._keep = ctrl
        return ctrl.solver, env._robot_state.clone().cuda()
    env = Navigation2DEnv()
    s = mppi_cls()(T, 65536, 3, 2, env.dynamics, env.cost_function, env.u_min, env.u_max, torch.tensor([0.5, 0.5]), 1.0, **kw)
    s._keep = env
    return s, env.reset().clone().cuda()


def mppi_cls():
    from pi_mpc.mppi import MPPI

    return MPPI


def loop(solver, x0, n):
    for _ in range(n):
        solver.forward(x0)
    torch.cuda.synchronize()


def best_of(solver, x0, rounds=3, n=50, warm=20):
    loop(solver, x0, warm)
    solver.set_option("timing", 2)
    solver.stage_times_ms()
    best, stage = None, None
    for _ in range(rounds):
        t0 = time.perf_counter()
        loop(solver, x0, n)
        dt = (time.perf_counter() - t0) / n
        st = solver.stage_times_ms()["rollout_cost"]
        if best is None or dt < best:
            best, stage = dt, st
    solver.set_option("timing", 0)
    return best * 1e6, stage * 1e3


def main():
    which = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = ("c3", "c2") if not which or which[0] == "both" else (which[0],)
    loop_only = "--loop-only" in sys.argv
    for w in which:
        rows = {}
        for on in (False, True):
            solver, x0 = build(w, **(dict(action_cost=True) if on else {}))
            if loop_only:
                loop(solver, x0, 70)
                continue
            rows[on] = best_of(solver, x0)
            if on:  # the comparator: a separate pass needs the noise as tiles first
                solver.set_option("noise_regen", 0)
                solver.set_option("timing", 1)
                loop(solver, x0, 20)
                solver.stage_times_ms()
                loop(solver, x0, 50)
                sample_us = solver.stage_times_ms()["sample"] * 1e3
                st = solver._stream()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                solver._h.call("mppi_add_action_cost", 1.0, st)
                ev[0].record()
                for _ in range(50):
                    solver._h.call("mppi_add_action_cost", 1.0, st)
                ev[1].record()
                torch.cuda.synchronize()
                rows["sample_us"], rows["pass_us"] = sample_us, ev[0].elapsed_time(ev[1]) * 1e3 / 50
            del solver
        if loop_only:
            continue
        (off_us, off_st), (on_us, on_st) = rows[False], rows[True]
        print(f"{w}: solve off {off_us:8.2f} us  on {on_us:8.2f} us  (+{on_us - off_us:6.2f} us, {100 * (on_us / off_us - 1):+.2f} %)   "
              f"rollout stage off {off_st:8.2f} us  on {on_st:8.2f} us  (+{on_st - off_st:6.2f} us)   "
              f"comparator: sample_kernel {rows['sample_us']:7.2f} us + separate pass (two launches) {rows['pass_us']:7.2f} us")


if __name__ == "__main__":
    main()
