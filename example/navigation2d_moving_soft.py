"""The scene of navigation2d_moving.py driven twice from the same seed at a SMALL sample count: with the hard disc model
("nav2d_discs": a disc costs w inside and nothing outside) and with the soft one ("nav2d_discs_soft": a graded skirt from
skirt * w at the rim to 0 at reach * radius, envs.SoftMovingObstacleNav2DEnv) (no rendering).

With few samples the hard rule only reacts once a sample lands inside a disc; the skirt makes keeping a distance cheaper than
grazing a rim before that.  Prints, for each model, the ticks, the ticks in collision and the minimum clearance to any disc
over the run (distance to the nearest rim, metres; negative: inside)."""
import torch

import _common  # noqa: F401  (puts mppi_playground_amd on the path)
from envs import MovingObstacleNav2DEnv, SoftMovingObstacleNav2DEnv
from navigation2d_moving import SEED, crossing_discs
from pi_mpc.mppi import MPPI

SETTINGS = dict(horizon=30, num_samples=256, dim_state=3, dim_control=2, lambda_="ESSPS")
RADIUS, REACH, SKIRT = 0.5, 2.0, 1.0


def clearance(world, pose) -> float:
    """distance from the robot to the nearest disc's rim where the discs are NOW (row 0 of the table)"""
    row = world._disc_table[0]
    d = torch.sqrt((pose[0] - row[:, 0]) ** 2 + (pose[1] - row[:, 1]) ** 2) - torch.sqrt(row[:, 2])
    return float(d.min())


def run(soft: bool, tick_limit: int = 500):
    """-> (arrived, ticks, ticks in collision, minimum clearance)"""
    if soft:
        world = SoftMovingObstacleNav2DEnv(horizon=SETTINGS["horizon"], soft_reach=REACH, soft_skirt=SKIRT, seed=SEED)
    else:
        world = MovingObstacleNav2DEnv(horizon=SETTINGS["horizon"], seed=SEED)
    world.set_moving_obstacles(*crossing_discs(), radius=RADIUS)
    mppi = MPPI(dynamics=world.dynamics, cost_func=world.cost_function, u_min=world.u_min, u_max=world.u_max,
                sigmas=torch.tensor([0.5, 0.5]), seed=SEED, **SETTINGS)
    assert mppi._model == ("nav2d_discs_soft" if soft else "nav2d_discs")
    pose, arrived, hit_ticks, closest = world.reset(), False, 0, float("inf")
    for tick in range(1, tick_limit + 1):
        plan, _ = mppi(pose)
        pose, arrived = world.step(plan[0])  # (moves the discs and rewrites the prediction in place)
        hit_ticks += int(world.collision_check(pose.view(1, 1, 3)).sum() > 0)
        closest = min(closest, clearance(world, pose))
        if arrived:
            break
    return bool(arrived), tick, hit_ticks, closest


if __name__ == "__main__":
    for soft in (False, True):
        arrived, ticks, hits, closest = run(soft)
        name = f"nav2d_discs_soft (reach {REACH}, skirt {SKIRT})" if soft else "nav2d_discs (hard)"
        print(f"{name}: {'goal reached' if arrived else 'goal NOT reached'} in {ticks} ticks, {hits} ticks in collision, "
              f"minimum clearance {closest:+.3f} m")
