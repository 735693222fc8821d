"""Navigation2DEnv with an UNCERTAIN start state, driven twice from one seed (no rendering).

Every tick the controller is handed not the true pose but an estimate drawn round it (position and heading noise, as a
localisation filter would deliver it).  Run 1 solves plainly on the estimate.  Run 2 also draws 8 particles round the same
estimate and hands them to set_state_particles(): every sampled control sequence is scored from every particle and the
solver keeps the mean of its 2 worst outcomes (risk="cvar", risk_alpha=0.25).  Both runs see the same estimates.

Prints, for each run, the ticks, the ticks the TRUE pose spent inside an obstacle and the minimum distance of the true pose to
any obstacle cell over the run (metres; 0: inside)."""
import math

import numpy as np
import torch

import _common  # noqa: F401  (puts mppi_playground_amd on the path)
from envs.navigation_2d import Navigation2DEnv
from pi_mpc.mppi import MPPI

SEED = 7
SETTINGS = dict(horizon=30, num_samples=1024, dim_state=3, dim_control=2, lambda_="ESSPS")
POS_STD, YAW_STD = 0.25, 0.10  # of the estimate round the true pose, and of the particles round the estimate
PARTICLES, ALPHA = 8, 0.25


def obstacle_cells(world) -> torch.Tensor:
    """centres [n, 2] of the occupied cells, in metres (a lookup rounds xy / cell + origin to the cell index)"""
    g = world._obstacle_map.grid_spec()
    ij = np.argwhere(np.asarray(g.cells) > 0).astype(np.float64)
    return torch.from_numpy((ij - np.asarray(g.origin, np.float64)) * float(g.cell_size)).float()


def run(particles: int, tick_limit: int = 500):
    """-> (arrived, ticks, ticks in collision, minimum distance to an obstacle cell)"""
    world = Navigation2DEnv()
    mppi = MPPI(dynamics=world.dynamics, cost_func=world.cost_function, u_min=world.u_min, u_max=world.u_max,
                sigmas=torch.tensor([0.5, 0.5]), seed=SEED, risk="cvar", risk_alpha=ALPHA, **SETTINGS)
    rng = np.random.default_rng(SEED)  # (one stream per run, consumed alike: both runs meet the same estimation errors)
    std = np.float32([POS_STD, POS_STD, YAW_STD])
    cells = obstacle_cells(world)
    pose, arrived, hit_ticks, closest = world.reset(), False, 0, math.inf
    for tick in range(1, tick_limit + 1):
        truth = pose.detach().cpu().numpy()
        estimate = (truth + rng.normal(0.0, 1.0, 3).astype(np.float32) * std).astype(np.float32)
        cloud = (estimate + rng.normal(0.0, 1.0, (PARTICLES, 3)).astype(np.float32) * std).astype(np.float32)
        if particles:
            mppi.set_state_particles(torch.from_numpy(cloud[:particles]))
        plan, _ = mppi(torch.from_numpy(estimate).to(pose.device))
        pose, arrived = world.step(plan[0])
        hit_ticks += int(world.collision_check(pose.view(1, 1, 3)).sum() > 0)
        closest = min(closest, float(torch.linalg.norm(cells - pose[:2].detach().cpu(), dim=1).min()))
        if arrived:
            break
    return bool(arrived), tick, hit_ticks, closest


if __name__ == "__main__":
    for particles in (0, PARTICLES):
        arrived, ticks, hits, closest = run(particles)
        name = f"{particles} particles, cvar (alpha {ALPHA})" if particles else "plain solve on the estimate"
        print(f"{name}: {'goal reached' if arrived else 'goal NOT reached'} in {ticks} ticks, {hits} ticks in collision, "
              f"minimum distance to an obstacle cell {closest:.3f} m")
