#!/usr/bin/env python3
"""What model ensembles cost (envs.MLPEnsemble: mlp41, two tanh layers of 32 units, one particle per network) against plain
learned-dynamics solves.  The numbers of profiles/r24_mlp_ensemble.md.

  1. N = 4096, T = 25: a plain solve, a solve with E = 5 members (set_model_particles("all")), and five plain solves —
     rollout stage (mppi_get_timing: the particle rollout plus the fold) and open-loop wall clock per solve.
  2. N = 2^20, T = 50: the rollout stage with E = 4 members against 4 x the plain stage.
  3. The member offset itself: one handle, P = 5 particles at the state, the map off (members=None), on, and on with every
     entry 0 (the offset mechanism without five different tables) — rollout stage, repetitions interleaved.
Every figure is the median over the solves of a repetition; --reps repetitions are printed with their spread.
`--plain-only` runs the plain solves alone (the parts a build without ensembles can run: the parent commit's numbers).
Usage: python scripts/mlp_ensemble_timing.py [--reps 5] [--plain-only | --only-offset]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch

import mppi_playground_amd  # noqa: F401
from envs import MLPModel
from pi_mpc.mppi import MPPI


def network(seed):
    """A contraction (every weight matrix at spectral norm 0.9, the residual output layer at 0.05): states stay bounded."""
    rng = np.random.default_rng(seed)
    dims = [5, 32, 32, 4]
    Ws = []
    for i, o in zip(dims[:-1], dims[1:]):
        W = rng.standard_normal((o, i))
        Ws.append((W * (0.9 / np.linalg.norm(W, 2))).astype(np.float32))
    Ws[-1] = (Ws[-1] * np.float32(0.05)).astype(np.float32)
    bs = [(0.1 * rng.standard_normal(o)).astype(np.float32) for o in dims[1:]]
    bs[-1] = (bs[-1] * np.float32(0.05)).astype(np.float32)
    return MLPModel(Ws, bs, activation="tanh", residual=True, goal=[0.2, -0.1, 0.3, 0.0], q=[1.0, 0.5, 2.0, 1.0], r=[0.05])


def build(N, T, members=0):
    if members:
        from envs import MLPEnsemble

        m = MLPEnsemble([network(e) for e in range(members)])
    else:
        m = network(0)
    solver = MPPI(horizon=T, num_samples=N, dim_state=4, dim_control=1, dynamics=m.dynamics, cost_func=m.cost,
                  u_min=torch.tensor([-1.5]), u_max=torch.tensor([1.5]), sigmas=torch.tensor([0.8]), lambda_=1.0)
    assert solver._model == "mlp41"
    solver._keep = m
    return solver, torch.tensor([0.3, -0.2, 0.5, 0.1], device="cuda")


def loop(solver, x0, n):
    for _ in range(n):
        solver.forward(x0)
    torch.cuda.synchronize()


def rollout_stage_us(solver, x0, n):
    """Median rollout-stage time over n solves (the stage is drained after every solve)."""
    solver.set_option("timing", 1)
    solver.stage_times_ms()
    vals = []
    for _ in range(n):
        solver.forward(x0)
        vals.append(solver.stage_times_ms()["rollout_cost"] * 1e3)
    solver.set_option("timing", 0)
    return statistics.median(vals)


def wall_us(solver, x0, n, warm):
    loop(solver, x0, warm)
    t0 = time.perf_counter()
    loop(solver, x0, n)
    return (time.perf_counter() - t0) / n * 1e6


def line(what, vals, unit="us"):
    print(f"{what:58s} " + "  ".join(f"{v:10.2f}" for v in vals) +
          f"  {unit}   median {statistics.median(vals):.2f}  spread {max(vals) - min(vals):.2f}", flush=True)


def measure(solver, x0, reps, n):
    loop(solver, x0, 10)
    stage = [rollout_stage_us(solver, x0, n) for _ in range(reps)]
    wall = [wall_us(solver, x0, n, 5) for _ in range(reps)]
    return stage, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--only-offset", action="store_true", help="part 3 alone")
    args = ap.parse_args()
    R = args.reps
    if not args.only_offset:
        parts_1_and_2(args, R)
    if not args.plain_only:
        part_3(R)


def parts_1_and_2(args, R):
    # 1. control-sized
    N, T = 4096, 25
    plain, x0 = build(N, T)
    ps, pw = measure(plain, x0, R, 40)
    line(f"1. N={N} T={T} plain solve: rollout stage", ps)
    line(f"1. N={N} T={T} plain solve: open loop", pw)
    line(f"1. N={N} T={T} five plain solves: open loop (5 x)", [5 * v for v in pw])
    if not args.plain_only:
        ens, _ = build(N, T, members=5)
        ens.set_model_particles("all")
        es, ew = measure(ens, x0, R, 40)
        line(f"1. N={N} T={T} E=5 members: rollout stage (+ fold)", es)
        line(f"1. N={N} T={T} E=5 members: open loop", ew)
        print(f"1. E=5 solve / plain solve = {statistics.median(ew) / statistics.median(pw):.2f}; / five plain solves = "
              f"{statistics.median(ew) / (5 * statistics.median(pw)):.2f}", flush=True)
        del ens
    del plain
    # 2. large
    N, T = 1 << 20, 50
    plain, x0 = build(N, T)
    loop(plain, x0, 3)
    ps = [rollout_stage_us(plain, x0, 8) for _ in range(R)]
    line(f"2. N=2^20 T={T} plain: rollout stage", ps)
    line(f"2. N=2^20 T={T} 4 x the plain rollout stage", [4 * v for v in ps])
    del plain
    if args.plain_only:
        return
    ens, _ = build(N, T, members=4)
    ens.set_model_particles("all")
    loop(ens, x0, 3)
    es = [rollout_stage_us(ens, x0, 8) for _ in range(R)]
    line(f"2. N=2^20 T={T} E=4 members: rollout stage (+ fold)", es)
    print(f"2. E=4 stage / (4 x plain stage) = {statistics.median(es) / (4 * statistics.median(ps)):.3f}", flush=True)
    del ens


def part_3(R):
    # the offset itself: one handle, the same five particles, the map off, on, and on with one member throughout (interleaved)
    for N, T in ((4096, 25), (1 << 20, 50)):
        ens, x0 = build(N, T, members=5)
        parts = x0.repeat(5, 1)
        off, on, same = [], [], []
        n = 40 if N < 100000 else 6
        for _ in range(R):
            for members, vals in ((None, off), (range(5), on), ([0] * 5, same)):
                ens.set_state_particles(parts, members=members)
                loop(ens, x0, 3)
                vals.append(rollout_stage_us(ens, x0, n))
        line(f"3. N={N} T={T} P=5 members=None: rollout stage (+ fold)", off)
        line(f"3. N={N} T={T} P=5 map [0..4]: rollout stage (+ fold)", on)
        line(f"3. N={N} T={T} P=5 map [0,0,0,0,0]: rollout stage (+ fold)", same)
        m = statistics.median
        print(f"3. N={N}: map - no map = {m(on) - m(off):+.2f} us, one-member map - no map = {m(same) - m(off):+.2f} us; "
              f"spread of the members=None repetitions {max(off) - min(off):.2f} us", flush=True)
        del ens


if __name__ == "__main__":
    main()
