"""Pendulum swing-up with an ENSEMBLE of learned dynamics: five bootstrap networks fitted to deliberately sparse data, the
plan judged under all of them (one particle per network, every rollout carried through one member).

The data cover only slow states (|thdot| <= 3 rad/s of the pendulum's [-8, 8]): away from them a single network is confidently
wrong, and the members of a bootstrap ensemble disagree.  Three swing-ups on the TRUE pendulum, same seed: the nominal network
alone, and set_model_particles("all") under the "mean" and the "cvar" measure.  A demonstration: it prints what each run does.
"""
import numpy as np
import torch

from _common import run_loop
from envs import MLPEnsemble
from envs.classic_control import pendulum_dynamics
from learned_pendulum import W_SCALE, features
from pi_mpc.mppi import MPPI

MEMBERS = 5


def sparse_data(samples: int = 300, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    th = (torch.rand(samples, generator=g) * 2 - 1) * np.pi
    w = (torch.rand(samples, generator=g) * 2 - 1) * 3.0  # slow states only
    u = (torch.rand(samples, 1, generator=g) * 2 - 1) * 2.0
    s = torch.stack((th, w), dim=1)
    x = torch.cat((features(s)[:, :3], u), dim=1)
    y = (features(pendulum_dynamics(s, u)) - features(s))[:, :3]
    return x, y


def fit_member(x, y, seed: int, steps: int = 400) -> torch.nn.Sequential:
    """One bootstrap member: a resample of the data with replacement, its own initialisation."""
    g = torch.Generator().manual_seed(1000 + seed)
    pick = torch.randint(0, len(x), (len(x),), generator=g)
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(4, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                              torch.nn.Linear(32, 3))
    opt = torch.optim.Adam(net.parameters(), lr=5e-3)
    for _ in range(steps):
        opt.zero_grad()
        loss = torch.mean((net(x[pick]) - y[pick]) ** 2)
        loss.backward()
        opt.step()
    return net


def disagreement(nets) -> float:
    """rms spread of the members' predictions on FAST states, which the data never showed."""
    g = torch.Generator().manual_seed(7)
    s = torch.stack(((torch.rand(512, generator=g) * 2 - 1) * np.pi, (torch.rand(512, generator=g) * 2 - 1) * 8.0), dim=1)
    x = torch.cat((features(s)[:, :3], (torch.rand(512, 1, generator=g) * 2 - 1) * 2.0), dim=1)
    with torch.no_grad():
        pred = torch.stack([n(x) for n in nets])
    return float(pred.std(dim=0).pow(2).mean().sqrt())


def swing_up(ens, label, steps, particles=None, **kw):
    solver = MPPI(horizon=30, num_samples=1000, dim_state=4, dim_control=1, dynamics=ens.dynamics, cost_func=ens.cost,
                  u_min=torch.tensor([-2.0]), u_max=torch.tensor([2.0]), sigmas=torch.tensor([1.0]), lambda_=0.5, **kw)
    assert solver._model == "mlp41", "the learned model runs fused"
    if particles is not None:
        solver.set_model_particles(particles)
    true = {"s": torch.tensor([[np.pi, 0.0]], device="cuda"), "up": 0}

    def step(_, u):  # the simulator is the true pendulum; the solver sees its features
        true["s"] = pendulum_dynamics(true["s"], u.view(1, -1))
        true["up"] += int(torch.cos(true["s"][0, 0]) > 0.95)
        return features(true["s"])[0]

    run_loop(solver, step, features(true["s"])[0], steps, label)
    th = float(torch.atan2(torch.sin(true["s"][0, 0]), torch.cos(true["s"][0, 0])))
    print(f"{label}: final angle from upright {th:+.3f} rad, angular velocity {float(true['s'][0, 1]):+.3f} rad/s, "
          f"{true['up']} of {steps} steps within 0.32 rad of upright")
    return th, true["up"]


def main(steps: int = 200):
    x, y = sparse_data()
    nets = [fit_member(x, y, e) for e in range(MEMBERS)]
    print(f"learned_pendulum_ensemble: {MEMBERS} bootstrap networks on {len(x)} slow transitions; rms disagreement on fast "
          f"states {disagreement(nets):.4f} (rms target on the data {float(torch.mean(y ** 2)) ** 0.5:.4f})")
    ens = MLPEnsemble.from_modules(nets, residual=True, goal=[1.0, 0.0, 0.0], q=[2.0, 0.5, 0.01 * W_SCALE ** 2], r=[0.001])
    out = {"nominal": swing_up(ens, "nominal network alone", steps)}
    out["mean"] = swing_up(ens, "ensemble, mean over members", steps, "all", risk="mean")
    out["cvar"] = swing_up(ens, "ensemble, CVaR(0.4) over members", steps, "all", risk="cvar", risk_alpha=0.4)
    return out


if __name__ == "__main__":
    main()
