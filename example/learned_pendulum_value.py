"""Pendulum swing-up with learned dynamics AND a learned terminal value: a short horizon closed by what a critic has learned
about everything behind it (TD-MPC, MPPI with a learned cost-to-go).

The dynamics network is the one of example/learned_pendulum.py.  The value network (3 -> 32 -> 32 -> 1, tanh) is fitted on the
CPU by a few sweeps of fitted value iteration over the FITTED model: on sampled states, V(s) <- min over a grid of torques of
c(s, u) + gamma * V(f(s, u)), regressed with Adam.  No data files, under a minute.  Its input is the model's own state
(cos th, sin th, thdot / 8): periodic in the angle, so nothing needs wrapping.

The swing-up runs from one seed three ways — T = 8 without the value, T = 8 with it, T = 30 without — and reports the ticks to
upright (the first tick from which |angle| < 0.3 rad holds to the end of the run) and the time per tick, as they come out.
"""
import time

import numpy as np
import torch

from _common import ROOT  # noqa: F401  (puts the package on sys.path)
from envs import MLPModel
from envs.classic_control import pendulum_dynamics
from learned_pendulum import W_SCALE, features, fit
from pi_mpc.mppi import MPPI

GOAL, Q, R = [1.0, 0.0, 0.0], [2.0, 0.5, 0.01 * W_SCALE ** 2], [0.001]
GAMMA = 0.97


def stage_cost(f: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """The model's quadratic on features [B, 3] and torques [B, 1]."""
    g, q = torch.tensor(GOAL), torch.tensor(Q)
    return ((f - g) ** 2 * q).sum(dim=1) + R[0] * u[:, 0] ** 2


def fit_value(model: MLPModel, sweeps: int = 30, samples: int = 2048, inner: int = 30, seed: int = 1, verbose: bool = True):
    """Fitted value iteration on the fitted model, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    th = (torch.rand(samples, generator=g) * 2 - 1) * np.pi
    w = (torch.rand(samples, generator=g) * 2 - 1) * 8.0
    s = features(torch.stack((th, w), dim=1))                      # [B, 4], the model's padded state
    torques = torch.linspace(-2.0, 2.0, 9)
    with torch.no_grad():                                          # the successors under every torque of the grid, once
        nxt = torch.stack([model.dynamics(s, torch.full((samples, 1), float(u))) for u in torques])     # [9, B, 4]
        cost = torch.stack([stage_cost(s[:, :3], torch.full((samples, 1), float(u))) for u in torques])  # [9, B]
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(3, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(), torch.nn.Linear(32, 1))
    opt = torch.optim.Adam(net.parameters(), lr=3e-3)
    for sweep in range(sweeps):
        with torch.no_grad():
            target = (cost + GAMMA * net(nxt[:, :, :3])[:, :, 0]).min(dim=0).values
        for _ in range(inner):
            opt.zero_grad()
            loss = torch.mean((net(s[:, :3])[:, 0] - target) ** 2)
            loss.backward()
            opt.step()
    if verbose:
        v = net(s[:, :3])[:, 0].detach()
        print(f"learned_pendulum_value: {sweeps} sweeps of fitted value iteration on {samples} states, last residual rms "
              f"{float(loss.detach()) ** 0.5:.3f}; V from {float(v.min()):.2f} (near upright) to {float(v.max()):.2f}")
    return net


def swing_up(model: MLPModel, horizon: int, with_value: bool, steps: int = 200, seed: int = 42):
    """-> (ticks to upright or None, ms per tick, final angle)"""
    solver = MPPI(horizon=horizon, num_samples=1000, dim_state=4, dim_control=1, dynamics=model.dynamics, cost_func=model.cost,
                  terminal_cost=model.terminal_cost if with_value else None, u_min=torch.tensor([-2.0]), u_max=torch.tensor([2.0]),
                  sigmas=torch.tensor([1.0]), lambda_=0.5, seed=seed)
    assert solver._model == "mlp41", "the learned model runs fused, with or without its value"
    true = torch.tensor([[np.pi, 0.0]], device="cuda")
    angles, total = [], 0.0
    for _ in range(steps):
        x = features(true)[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        action_seq, _ = solver.forward(state=x)
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
        true = pendulum_dynamics(true, action_seq[0].view(1, -1))
        angles.append(abs(float(torch.atan2(torch.sin(true[0, 0]), torch.cos(true[0, 0])))))
    up = np.asarray(angles) < 0.3
    away = np.nonzero(~up)[0]
    first = 0 if len(away) == 0 else int(away[-1]) + 1
    return (first if first < steps else None), total / steps * 1e3, angles[-1]


def main(steps: int = 200):
    net = fit()
    model = MLPModel.from_module(net, residual=True, goal=GOAL, q=Q, r=R)
    t0 = time.perf_counter()
    model.set_value_module(fit_value(model), weight=1.0)
    print(f"learned_pendulum_value: value fitted in {time.perf_counter() - t0:.1f} s")
    out = {}
    for label, T, use in (("T=8 without the value", 8, False), ("T=8 with the value", 8, True), ("T=30 without the value", 30, False)):
        ticks, ms, angle = swing_up(model, T, use, steps)
        out[label] = (ticks, ms, angle)
        reached = f"upright from tick {ticks}" if ticks is not None else f"NOT upright within {steps} ticks"
        print(f"learned_pendulum_value: {label}: {reached}; {ms:.3f} ms per tick; final angle from upright {angle:.3f} rad")
    return out


if __name__ == "__main__":
    main()
