"""The planar quadrotor of example/learned_quadrotor2d.py as a TRACKING controller: the same kind of learned network (an
MLPModel8 fitted to the vehicle's transitions, native model "mlp82"), the pitch declared angular, and a reference that moves —
a figure-of-eight, one row per horizon step, shifted by one row every tick (MLPModel8.set_reference: the table is rewritten
in place on the device, nothing is rebuilt and nothing waits for the host).

    reference of tick i, step t:  p(tau) = (1.2 * sin(tau), 1.0 + 0.6 * sin(2 * tau)),  tau = W * DT * (i + t)
    its rows carry the position and the path's velocity (scaled as the network sees them); pitch, pitch rate: 0

The last row's weights are doubled: the terminal cost reads row T - 1 (there is no row T), so the weight of the end of the
horizon goes there and counts for the state of step T - 1 and for the final state.
Prints the RMS position error over the last 100 ticks and the time per tick.
"""
import math
import time

import numpy as np
import torch

import _common  # noqa: F401  (puts the package on sys.path)
from envs import MLPModel8
from learned_quadrotor2d import DT, SCALE, fit, quadrotor_step
from pi_mpc.mppi import MPPI

W = 0.8         # rad / s along the figure
HORIZON = 30


def figure_rows(first_tick: int, rows: int, device) -> torch.Tensor:
    """[rows, 6] goals in the network's scaled state for ticks first_tick .. first_tick + rows - 1."""
    tau = W * DT * torch.arange(first_tick, first_tick + rows, device=device, dtype=torch.float32)
    x, z = 1.2 * torch.sin(tau), 1.0 + 0.6 * torch.sin(2 * tau)
    vx, vz = 1.2 * W * torch.cos(tau), 1.2 * W * torch.cos(2 * tau)
    zero = torch.zeros_like(tau)
    return torch.stack((x, z, zero, vx, vz, zero), dim=1) / SCALE.to(device)


def main(steps: int = 400):
    net = fit()
    q = torch.tensor([6.0, 6.0, 0.5, 0.3 * 9.0, 0.3 * 9.0, 0.05 * 9.0])
    model = MLPModel8.from_module(net, residual=True, q=q.tolist(), r=[0.05, 0.05], angular=[2])  # the pitch is an angle
    solver = MPPI(horizon=HORIZON, num_samples=1000, dim_state=model.dim_state, dim_control=2, dynamics=model.dynamics,
                  cost_func=model.cost, u_min=torch.tensor([-1.0, -1.0]), u_max=torch.tensor([1.0, 1.0]),
                  sigmas=torch.tensor([0.4, 0.4]), lambda_=0.5)
    assert solver._model == "mlp82", "the learned model runs fused"
    dev = torch.device("cuda")
    weights = q.to(dev).repeat(HORIZON, 1)
    weights[-1] *= 2.0  # the end of the horizon: row T - 1 counts for step T - 1 and for the final state
    model.set_reference(figure_rows(0, HORIZON, dev), weights)  # a device table: later ticks rewrite it in place
    table = model.reference
    scale = SCALE.to(dev)
    s = torch.tensor([[0.0, 1.0, 0.0, 0.0, 0.0, 0.0]], device=dev)  # the figure's centre, at rest
    errors, total = [], 0.0
    for i in range(steps):
        table[:, :6] = figure_rows(i, HORIZON, dev)  # shifted by one row every tick
        model.reference_changed()
        torch.cuda.synchronize()
        t0 = time.time()
        action_seq, _ = solver.forward(state=model.pad_state(s[0] / scale))
        torch.cuda.synchronize()
        total += time.time() - t0
        assert model.reference is table
        s = quadrotor_step(s, action_seq[0].view(1, -1))
        tau = W * DT * (i + 1)
        errors.append(math.hypot(float(s[0, 0]) - 1.2 * math.sin(tau), float(s[0, 1]) - (1.0 + 0.6 * math.sin(2 * tau))))
    rms = float(np.sqrt(np.mean(np.square(errors[-100:]))))
    print(f"learned_quadrotor2d_tracking: RMS position error over the last 100 ticks {rms:.3f} m, pitch "
          f"{float(s[0, 2]):+.3f} rad, average solve time {total / steps * 1e3:.3f} ms over {steps} ticks")
    return rms


if __name__ == "__main__":
    main()
