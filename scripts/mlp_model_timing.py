#!/usr/bin/env python3
"""What a learned-dynamics solve costs (envs.MLPModel: mlp41, two tanh layers of 32 units) fused, and the same network on the
generic path with graph_callables=True — the number the native model exists to beat.

Per size (N, T): stage times of the fused solve from mppi_get_timing (option "timing" = 1, drained after every solve; the
median over the solves, per repetition), its open-loop wall clock per solve with timing off, and the wall clock per solve of
the generic path after its graph capture.  With --profile-loop N the script only runs N fused solves at the first size (the
command to put behind `rocprofv3 --kernel-trace --stats --` for the rollout kernel's own time).
Usage: python scripts/mlp_model_timing.py [--sizes 1048576x50,4096x25] [--reps 3] [--skip-generic]"""
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

STAGES = ("sample", "rollout_cost", "weights_reduce", "finalize")


def network(seed=0):
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


def build(N, T, tag=True, **kw):
    m = network()
    dyn, cost = (m.dynamics, m.cost) if tag else ((lambda s, a: m.dynamics(s, a)), (lambda s, a, i: m.cost(s, a, i)))
    solver = MPPI(horizon=T, num_samples=N, dim_state=4, dim_control=1, dynamics=dyn, cost_func=cost,
                  u_min=torch.tensor([-1.5]), u_max=torch.tensor([1.5]), sigmas=torch.tensor([0.8]), lambda_=1.0, **kw)
    assert (solver._model == "mlp41") == tag
    solver._keep = m
    return solver, torch.tensor([0.3, -0.2, 0.5, 0.1], device="cuda")


def loop(solver, x0, n):
    for _ in range(n):
        solver.forward(x0)
    torch.cuda.synchronize()


def wall(solver, x0, n, warm):
    loop(solver, x0, warm)
    t0 = time.perf_counter()
    loop(solver, x0, n)
    return (time.perf_counter() - t0) / n * 1e6


def fused(N, T, n=40, warm=10):
    solver, x0 = build(N, T)
    loop(solver, x0, warm)
    solver.set_option("timing", 1)
    solver.stage_times_ms()
    per = {s: [] for s in STAGES}
    for _ in range(n):
        solver.forward(x0)
        t = solver.stage_times_ms()
        for s in STAGES:
            per[s].append(t[s] * 1e3)
    solver.set_option("timing", 0)
    return [statistics.median(per[s]) for s in STAGES] + [wall(solver, x0, n, warm)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576x50,4096x25")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-generic", action="store_true")
    ap.add_argument("--profile-loop", type=int, default=0)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    if args.profile_loop:
        solver, x0 = build(*sizes[0])
        loop(solver, x0, args.profile_loop)
        return
    for N, T in sizes:
        rows = [fused(N, T) for _ in range(args.reps)]
        for col, what in enumerate(STAGES + ("open loop",)):
            vals = [r[col] for r in rows]
            print(f"mlp41 fused   N={N:8d} T={T:3d} {what:15s} " + "  ".join(f"{v:10.2f}" for v in vals) +
                  f"  us   (spread {max(vals) - min(vals):.2f})", flush=True)
        # arithmetic floor of the rollout: multiply-adds x sample-steps / 64 lanes at the VALU issue peak
        floor_us = 1312.0 * N * T / 64.0 / 1.2288e12 * 1e6
        ro = statistics.median(r[1] for r in rows)
        print(f"mlp41 fused   N={N:8d} T={T:3d} rollout floor   {floor_us:10.2f}  us   -> {floor_us / ro:.3f} of the VALU issue peak", flush=True)
        if args.skip_generic:
            continue
        solver, x0 = build(N, T, tag=False, graph_callables=True)
        loop(solver, x0, 3)  # eager warm-up, capture, first replay
        vals = [wall(solver, x0, 5 if N > 100000 else 30, 1) for _ in range(args.reps)]
        print(f"mlp41 generic N={N:8d} T={T:3d} graph state {solver._graph_state}: open loop " +
              "  ".join(f"{v:10.1f}" for v in vals) + f"  us   (spread {max(vals) - min(vals):.1f})", flush=True)
        del solver


if __name__ == "__main__":
    main()
