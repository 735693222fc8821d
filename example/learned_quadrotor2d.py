"""A planar quadrotor flown to a hover point with LEARNED dynamics: a two-hidden-layer tanh network is fitted to transitions of
the equations below and handed to the solver as an MLPModel8 — six states and two thrusts, more than the 4-state MLPModel
takes; the network runs inside the fused rollout kernels (native model "mlp82").

The vehicle (the simulator and the source of the training data; semi-implicit Euler, DT = 0.05 s):
    state (x, z, th, vx, vz, w): position, pitch, their rates;  thrusts f1, f2 in units of half the weight (hover: 1, 1)
    vx += DT * (-G * (f1 + f2) / 2 * sin th)      vz += DT * (G * (f1 + f2) / 2 * cos th - G)      w += DT * K * (f1 - f2)
    x  += DT * vx                                 z  += DT * vz                                     th += DT * w
The solver's controls are the thrusts' deviations from hover, u = f - 1 in [-1, 1], so that the quadratic control cost pulls
towards hovering and not towards falling.  The learned model sees the state scaled to order one, (x, z, th, vx / 3, vz / 3,
w / 3), padded to the eight components the native model takes (MLPModel8.pad_state); the network predicts the change of the
six.  A few hundred Adam steps on the CPU, no data files.
"""
import numpy as np
import torch

from _common import run_loop
from envs import MLPModel8
from pi_mpc.mppi import MPPI

DT, G, K = 0.05, 9.81, 12.0
SCALE = torch.tensor([1.0, 1.0, 1.0, 3.0, 3.0, 3.0])  # the network sees state / SCALE


def quadrotor_step(s: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """[B, 6] state, [B, 2] thrust deviations from hover -> [B, 6] the state DT later."""
    x, z, th, vx, vz, w = s.unbind(dim=1)
    f1, f2 = 1.0 + u[:, 0], 1.0 + u[:, 1]
    a = G * (f1 + f2) / 2
    vx = vx + DT * (-a * torch.sin(th))
    vz = vz + DT * (a * torch.cos(th) - G)
    w = w + DT * K * (f1 - f2)
    return torch.stack((x + DT * vx, z + DT * vz, th + DT * w, vx, vz, w), dim=1)


def fit(steps: int = 800, samples: int = 8192, seed: int = 0, verbose: bool = True) -> torch.nn.Sequential:
    """Fit the change of the scaled state on random transitions of quadrotor_step."""
    g = torch.Generator().manual_seed(seed)
    span = torch.tensor([2.0, 2.0, 1.2, 3.0, 3.0, 4.0])
    s = (torch.rand(samples, 6, generator=g) * 2 - 1) * span
    u = torch.rand(samples, 2, generator=g) * 2 - 1
    x = torch.cat((s / SCALE, u), dim=1)
    y = (quadrotor_step(s, u) - s) / SCALE
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(8, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                              torch.nn.Linear(32, 6))
    opt = torch.optim.Adam(net.parameters(), lr=5e-3)
    for i in range(steps):
        opt.zero_grad()
        loss = torch.mean((net(x) - y) ** 2)
        loss.backward()
        opt.step()
    if verbose:
        print(f"learned_quadrotor2d: fitted {samples} transitions in {steps} Adam steps, rms error "
              f"{float(loss.detach()) ** 0.5:.4f} (rms target {float(torch.mean(y ** 2)) ** 0.5:.4f})")
    return net


def main(steps: int = 200):
    net = fit()
    hover = [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]  # the point to reach and stay at, in the network's scaled state
    model = MLPModel8.from_module(net, residual=True, goal=hover, q=[4.0, 4.0, 1.0, 0.5 * 9.0, 0.5 * 9.0, 0.05 * 9.0],
                                  r=[0.05, 0.05])
    solver = MPPI(horizon=30, num_samples=1000, dim_state=model.dim_state, dim_control=2, dynamics=model.dynamics,
                  cost_func=model.cost, u_min=torch.tensor([-1.0, -1.0]), u_max=torch.tensor([1.0, 1.0]),
                  sigmas=torch.tensor([0.4, 0.4]), lambda_=0.5)
    assert solver._model == "mlp82", "the learned model runs fused"
    true = {"s": torch.zeros(1, 6, device="cuda")}
    scale = SCALE.cuda()

    def step(_, u):  # the simulator is the true vehicle; the solver sees its scaled, padded state
        true["s"] = quadrotor_step(true["s"], u.view(1, -1))
        return model.pad_state(true["s"][0] / scale)

    run_loop(solver, step, model.pad_state(true["s"][0] / scale), steps, "learned_quadrotor2d")
    s = true["s"][0].tolist()
    dist = float(np.hypot(s[0] - hover[0], s[1] - hover[1]))
    print(f"learned_quadrotor2d: final distance from the hover point {dist:.3f} m, pitch {s[2]:+.3f} rad, "
          f"speed {float(np.hypot(s[3], s[4])):.3f} m/s")
    return dist


if __name__ == "__main__":
    main()
