"""Pendulum swing-up with LEARNED dynamics: a two-layer tanh network is fitted to transitions of the shipped pendulum model
and handed to the solver as an MLPModel — its weights are data, the network runs inside the fused rollout kernels.

State of the learned model: (cos th, sin th, thdot / 8), padded to the four components the native model takes; the network
predicts the change of the three.  A few hundred Adam steps on the CPU, no data files.  The simulator stays the true model.
"""
import numpy as np
import torch

from _common import run_loop
from envs import MLPModel
from envs.classic_control import pendulum_dynamics
from pi_mpc.mppi import MPPI

W_SCALE = 8.0  # thdot lies in [-8, 8]: the network sees thdot / 8


def features(state: torch.Tensor) -> torch.Tensor:
    """[B, 2] (th, thdot) -> [B, 4] (cos th, sin th, thdot / 8, 0)."""
    th, w = state[:, 0], state[:, 1]
    return torch.stack((torch.cos(th), torch.sin(th), w / W_SCALE, torch.zeros_like(th)), dim=1)


def fit(steps: int = 600, samples: int = 4096, seed: int = 0, verbose: bool = True) -> torch.nn.Sequential:
    """Fit next_features - features on random transitions of the shipped model."""
    g = torch.Generator().manual_seed(seed)
    th = (torch.rand(samples, generator=g) * 2 - 1) * np.pi
    w = (torch.rand(samples, generator=g) * 2 - 1) * 8.0
    u = (torch.rand(samples, 1, generator=g) * 2 - 1) * 2.0
    s = torch.stack((th, w), dim=1)
    x = torch.cat((features(s)[:, :3], u), dim=1)
    y = (features(pendulum_dynamics(s, u)) - features(s))[:, :3]
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(4, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                              torch.nn.Linear(32, 3))
    opt = torch.optim.Adam(net.parameters(), lr=5e-3)
    for i in range(steps):
        opt.zero_grad()
        loss = torch.mean((net(x) - y) ** 2)
        loss.backward()
        opt.step()
    if verbose:
        print(f"learned_pendulum: fitted {samples} transitions in {steps} Adam steps, rms error "
              f"{float(loss.detach()) ** 0.5:.4f} (rms target {float(torch.mean(y ** 2)) ** 0.5:.4f})")
    return net


def main(steps: int = 200):
    net = fit()
    # upright is th = 0: cos = 1, sin = 0.  The quadratic in the features is flat at the bottom (both gradients vanish at
    # th = pi), so the height term carries most of the weight and the velocity term little: 2 (cos - 1)^2 + 0.5 sin^2
    # + 0.01 thdot^2 over a 1.5 s horizon lets the sampler find the pumping swings.
    model = MLPModel.from_module(net, residual=True, goal=[1.0, 0.0, 0.0], q=[2.0, 0.5, 0.01 * W_SCALE ** 2], r=[0.001])
    solver = MPPI(horizon=30, num_samples=1000, dim_state=4, dim_control=1, dynamics=model.dynamics, cost_func=model.cost,
                  u_min=torch.tensor([-2.0]), u_max=torch.tensor([2.0]), sigmas=torch.tensor([1.0]), lambda_=0.5)
    assert solver._model == "mlp41", "the learned model runs fused"
    true = {"s": torch.tensor([[np.pi, 0.0]], device="cuda")}

    def step(_, u):  # the simulator is the true pendulum; the solver sees its features
        true["s"] = pendulum_dynamics(true["s"], u.view(1, -1))
        return features(true["s"])[0]

    run_loop(solver, step, features(true["s"])[0], steps, "learned_pendulum")
    th = float(torch.atan2(torch.sin(true["s"][0, 0]), torch.cos(true["s"][0, 0])))
    print(f"learned_pendulum: final angle from upright {th:+.3f} rad, angular velocity {float(true['s'][0, 1]):+.3f} rad/s")
    return th


if __name__ == "__main__":
    main()
