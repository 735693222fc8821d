#!/usr/bin/env python3
"""What the 8-state learned-dynamics models cost (envs.MLPModel8: mlp82 and mlp84, two tanh layers of 32 units, residual)
against mlp42 and against the same network on the generic path.  The numbers of profiles/r25_mlp8.md.

Per size (N = 4096, T = 25 and N = 2^20, T = 50) and model:
  the fused path    rollout stage (mppi_get_timing) and open-loop wall clock per solve;
  the generic path  the same callables behind plain lambdas with graph_callables=True: open-loop wall clock per solve.
At the large size (the multi-kernel sequence) the finalize stage is printed too: it holds the batch-1 rollout of the state
sequence, T dependent network steps on one lane.
Every figure is the median over the solves of a repetition; --reps repetitions are printed with their spread.
`--plain-only` runs mlp42 alone (what a build without the 8-state ids can run: the parent commit's numbers).
Usage: python scripts/mlp8_timing.py [--reps 5] [--plain-only] [--no-generic]"""
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
import envs
from pi_mpc.mppi import MPPI

LIMITS = {2: ([-1.0, -2.0], [1.5, 2.0], [0.6, 1.0]), 4: ([-1.0, -2.0, -0.5, -1.5], [1.5, 2.0, 0.75, 1.0], [0.6, 1.0, 0.4, 0.7])}
X0 = [0.3, -0.2, 0.5, 0.1, -0.4, 0.25, 0.15, -0.1]


def network(name, seed=0):
    """A contraction (every weight matrix at spectral norm 0.9, the residual output layer at 0.05): states stay bounded."""
    ds, dc = int(name[3]), int(name[4])
    rng = np.random.default_rng(seed)
    dims = [ds + dc, 32, 32, ds]
    Ws = []
    for i, o in zip(dims[:-1], dims[1:]):
        W = rng.standard_normal((o, i))
        Ws.append((W * (0.9 / np.linalg.norm(W, 2))).astype(np.float32))
    Ws[-1] = (Ws[-1] * np.float32(0.05)).astype(np.float32)
    bs = [(0.1 * rng.standard_normal(o)).astype(np.float32) for o in dims[1:]]
    bs[-1] = (bs[-1] * np.float32(0.05)).astype(np.float32)
    cls = envs.MLPModel if ds == 4 else envs.MLPModel8
    return cls(Ws, bs, activation="tanh", residual=True, goal=[0.1] * ds, q=[1.0] * ds, r=[0.05] * dc)


def build(name, N, T, generic=False):
    m = network(name)
    ds, dc = int(name[3]), int(name[4])
    dyn, cost = (m.dynamics, m.cost) if not generic else ((lambda s, a: m.dynamics(s, a)), (lambda s, a, i: m.cost(s, a, i)))
    lo, hi, sig = LIMITS[dc]
    solver = MPPI(horizon=T, num_samples=N, dim_state=ds, dim_control=dc, dynamics=dyn, cost_func=cost, u_min=torch.tensor(lo),
                  u_max=torch.tensor(hi), sigmas=torch.tensor(sig), lambda_=1.0, **(dict(graph_callables=True) if generic else {}))
    assert solver._model == (None if generic else name)
    solver._keep = m
    return solver, torch.tensor(X0[:ds], device="cuda")


def loop(solver, x0, n):
    for _ in range(n):
        solver.forward(x0)
    torch.cuda.synchronize()


def stage_us(solver, x0, n, stage="rollout_cost"):
    """Median stage time over n solves (the stage is drained after every solve)."""
    solver.set_option("timing", 1)
    solver.stage_times_ms()
    vals = []
    for _ in range(n):
        solver.forward(x0)
        t = solver.stage_times_ms()
        vals.append(t[stage] * 1e3)
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
    return statistics.median(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--no-generic", action="store_true")
    args = ap.parse_args()
    R = args.reps
    names = ["mlp42"] if args.plain_only else ["mlp42", "mlp82", "mlp84"]
    for N, T, n in ((4096, 25, 40), (1 << 20, 50, 8)):
        tag = f"N={N} T={T}"
        fused = {}
        for name in names:
            solver, x0 = build(name, N, T)
            loop(solver, x0, 10 if N < 100000 else 3)
            line(f"{tag} {name} fused: rollout stage", [stage_us(solver, x0, n) for _ in range(R)])
            if N > 4096:
                line(f"{tag} {name} fused: finalize stage", [stage_us(solver, x0, n, "finalize") for _ in range(R)])
            fused[name] = line(f"{tag} {name} fused: open loop", [wall_us(solver, x0, n, 3) for _ in range(R)])
            del solver
        if args.plain_only or args.no_generic:
            continue
        for name in names[1:]:
            solver, x0 = build(name, N, T, generic=True)
            loop(solver, x0, 4)  # (warm-up, capture, two replays)
            assert solver._graph_state == "replay", solver._graph_state
            g = line(f"{tag} {name} generic, graph_callables: open loop", [wall_us(solver, x0, n if N < 100000 else 3, 1) for _ in range(R)])
            print(f"{tag} {name}: generic / fused = {g / fused[name]:.1f}", flush=True)
            del solver
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
