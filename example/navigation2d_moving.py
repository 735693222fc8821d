"""Drive the unicycle of MovingObstacleNav2DEnv to its goal through the static map while discs cross its way (no rendering).

The discs move at constant velocity; every tick the env predicts where each will be at every step of the horizon and the
solver tests step t of every sample against row t of that table, fused on the device (model "nav2d_discs").  Prints the
ticks, the time per tick and the number of ticks the robot spent inside a disc or a static obstacle."""
import math
import time

import torch

import _common  # noqa: F401  (puts mppi_playground_amd on the path)
from envs import MovingObstacleNav2DEnv
from pi_mpc.mppi import MPPI

SETTINGS = dict(horizon=30, num_samples=3000, dim_state=3, dim_control=2, lambda_="ESSPS")
SEED = 42


def crossing_discs(count: int = 6, speed: float = 0.6, cruise: float = 1.6):
    """Discs that reach the start-goal diagonal about when a robot cruising at `cruise` m/s does, from alternating sides."""
    h = (math.cos(math.pi / 4), math.sin(math.pi / 4))
    n = (-h[1], h[0])
    pos, vel = [], []
    for k in range(count):
        along = 4.0 + 3.5 * k           # where it crosses, metres from the start along the diagonal
        side = 1.0 if k % 2 == 0 else -1.0
        off = side * speed * along / cruise
        pos.append([-9.0 + along * h[0] + off * n[0], -9.0 + along * h[1] + off * n[1]])
        vel.append([-side * speed * n[0], -side * speed * n[1]])
    return torch.tensor(pos), torch.tensor(vel)


def run(tick_limit: int = 500) -> bool:
    world = MovingObstacleNav2DEnv(horizon=SETTINGS["horizon"], seed=SEED)
    world.set_moving_obstacles(*crossing_discs(), radius=0.5)
    mppi = MPPI(dynamics=world.dynamics, cost_func=world.cost_function, u_min=world.u_min, u_max=world.u_max,
                sigmas=torch.tensor([0.5, 0.5]), seed=SEED, **SETTINGS)
    assert mppi._model == "nav2d_discs"
    pose, arrived, hit_ticks, t0 = world.reset(), False, 0, None
    for tick in range(1, tick_limit + 1):
        if tick == 2:  # (the first tick pays the one-time set-up: module load, buffers, map rasterisation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        plan, _ = mppi(pose)
        pose, arrived = world.step(plan[0])  # (moves the discs and rewrites the prediction in place)
        hit_ticks += int(world.collision_check(pose.view(1, 1, 3)).sum() > 0)
        if arrived:
            break
    torch.cuda.synchronize()
    per_tick = (time.perf_counter() - t0) / max(tick - 1, 1) * 1e3 if t0 is not None else float("nan")
    print(f"{'Goal Reached!' if arrived else 'goal NOT reached'} {tick} ticks, {per_tick:.3f} ms per tick after the first, "
          f"{hit_ticks} ticks in collision; final state {pose.tolist()}")
    return bool(arrived) and hit_ticks == 0


if __name__ == "__main__":
    raise SystemExit(0 if run() else 1)
