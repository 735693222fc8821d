"""The racing example's loop with three slower cars ahead (no rendering).

The cars follow the centre line at their own constant speed, each a little to one side of it, so that the centre line is
blocked and a passage stays open inside the lane corridor on the other side.  Every tick the env predicts where each car will
be at every step of the horizon and the solver tests step t of every sample against row t of that table, fused on the device
(model "racing_discs").  Prints the ticks, the time per tick and the number of ticks the ego car spent inside another car.

`run(opponent_aware=False)` drives the same loop — same seed, same cars on the track — with the plain "racing" solver, which
does not see them."""
import time

import torch

import _common  # noqa: F401  (puts mppi_playground_amd on the path)
from envs.racing_controller import racing_controller
from envs.racing_env import RacingEnv
from envs.racing_opponents import OpponentRacingEnv, opponent_racing_controller

SETTINGS = dict(horizon=25, num_samples=4000)  # the racing example's size
SEED = 42
# centre-line index now (0.1 m apart), speed (m/s), radius (m), offset to the left of the centre line (m): the cars cover
# the centre line and leave more than 2 m of the 5.2 m lane corridor free on the other side
CARS = dict(path_index=[150, 300, 450], speed=[2.5, 2.5, 2.5], radius=0.9, lateral_offset=[0.4, -0.4, 0.4])
TICKS = 160  # enough to reach and pass all three


def run(ticks: int = TICKS, opponent_aware: bool = True, verbose: bool = True):
    """-> (ticks in collision with a car, ticks in collision with the static map, final path index)"""
    env = OpponentRacingEnv(horizon=SETTINGS["horizon"], seed=SEED)
    env.set_opponents(**CARS)
    if opponent_aware:
        controller = opponent_racing_controller(env, seed=SEED, **SETTINGS)
        assert controller.solver._model == "racing_discs"
    else:  # the plain racing model of the same track (the same seed builds the same maps): it knows no cars
        controller = racing_controller(RacingEnv(seed=SEED), seed=SEED, **SETTINGS)
        assert controller.solver._model == "racing"
    controller.set_cost_map(env._obstacle_map, env._lane_map)
    state = env.reset()
    car_ticks = map_ticks = 0
    t0 = None
    for tick in range(1, ticks + 1):
        if tick == 2:  # (the first tick pays the one-time set-up: module load, buffers, map rasterisation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        action_seq, _ = controller.update(state, env.racing_center_path)
        state, reached = env.step(action_seq[0, :])  # (moves the cars and rewrites the prediction in place)
        car_ticks += int(env.opponent_hits(state.view(1, 4)).sum() > 0)
        map_ticks += int(static_hits(env, state) > 0)
        if reached:
            break
    torch.cuda.synchronize()
    per_tick = (time.perf_counter() - t0) / max(tick - 1, 1) * 1e3 if t0 is not None else float("nan")
    index = controller.current_path_index
    if verbose:
        print(f"{'racing_discs' if opponent_aware else 'racing (blind)'}: {tick} ticks, {per_tick:.3f} ms per tick after the first, "
              f"{car_ticks} ticks inside a car, {map_ticks} inside a static obstacle; path index {index}, "
              f"cars at {[int(i) for i in env.opponent_path_indices()[0].tolist()]}; final state {state.tolist()}")
    return car_ticks, map_ticks, index


def static_hits(env, state) -> float:
    """the parent's static-map test for the one state"""
    return float(RacingEnv.collision_check(env, state.view(1, 1, 4)).sum())


if __name__ == "__main__":
    hit, _, _ = run()
    raise SystemExit(0 if hit == 0 else 1)
