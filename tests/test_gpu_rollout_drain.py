"""The regenerating horizon loop of rollout_cost_kernel is walked in two halves at two wave priorities (csrc/mppi_rollout.hpp,
trajectory_cost: "Even drain") on a real MI355X.  The tile-mode loop (`noise_regen` = 0) is untouched and is the in-tree reference:
costs, action sequence and state sequence of `noise_regen` = 1 must equal it bit for bit on a pair of handles with equal seeds.

Shapes: the horizons at which the halves are empty or unequal (racing has two steps per group: T = 1 .. 5, 7 give 0 .. 3 full
groups, with and without a ragged step behind them; T = 50 is the benchmark's), at N = 64 (one wave) and N = 8192 + 37 (a last
tile partly past the end, a last block with fewer than four live waves); and at T = 8 every copy of the loop: a start outside
the position clamp, a general wheel base, nav2d, a one-control model with a ragged last group, the cart-pole with its
per-lane redo, the rider block of a lazy state sequence and a stamped launch.
"""
import pytest
import torch

from test_gpu_covariance import _need_gpu, make

pytestmark = pytest.mark.gpu

N_RAGGED = 8192 + 37


def solves(solver, x0, regen, steps=2, **options):
    """`steps` solves from x0 (the second one warm-started, at the next solve index): (costs, actions, states) of each."""
    solver.set_option("noise_regen", regen)
    solver.set_option("fused_solve", 0)  # (the rollout kernel is the subject; the single-launch solve has its own loop)
    for name, value in options.items():
        solver.set_option(name, value)
    x0, out = x0.cuda(), []
    for _ in range(steps):
        a, s = solver.forward(x0)
        out.append((solver._costs.clone(), a.clone(), torch.as_tensor(s).clone()))
    torch.cuda.synchronize()
    return out


def assert_same_bits(regen, tiles):
    assert len(regen) == len(tiles)
    for k, (got, want) in enumerate(zip(regen, tiles)):
        for name, x, y in zip(("costs", "action_seq", "state_seq"), got, want):
            assert torch.isfinite(y).all(), (k, name)
            assert torch.equal(x, y), (k, name, int((x != y).sum()))


def check(build, steps=2, **options):
    """build() -> (solver, x0), called once per noise mode: equal seeds, equal everything."""
    outs = []
    for regen in (1, 0):
        solver, x0 = build()
        outs.append(solves(solver, x0, regen, steps, **options))
    assert_same_bits(*outs)


@pytest.mark.parametrize("N", [64, N_RAGGED])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 50])
def test_racing_halves_of_every_length(T, N):
    check(lambda: make("racing", T, N, 1.0))


def test_start_outside_the_position_clamp():
    """x0 beyond the map's edge: the copy of the loop whose first stage cost takes the bounds-tested lookup."""
    def build():
        solver, x0 = make("racing", 8, N_RAGGED, 1.0)
        x0 = x0.clone()
        x0[0] = 41.5  # (the map spans +-40 m)
        return solver, x0
    check(build)


def test_general_wheel_base():
    def build():
        _need_gpu()
        from envs.racing_controller import racing_controller
        from envs.racing_env import RacingEnv

        env = RacingEnv()
        env.L = torch.tensor(1.3, device=env.L.device, dtype=env.L.dtype)
        ctrl = racing_controller(env, horizon=8, num_samples=N_RAGGED, lambda_=1.0)
        ctrl.set_cost_map(env._obstacle_map, env._lane_map)
        ref, _ = ctrl.calc_ref_trajectory(env._robot_state, env.racing_center_path, 0, 8, DL=0.1, lookahead_distance=3,
                                          reference_path_interval=0.85)
        ctrl.set_reference(ref)
        ctrl.solver._test_keep = ctrl
        return ctrl.solver, env._robot_state.clone()
    check(build)


@pytest.mark.parametrize("model,T", [("nav2d", 8), ("pendulum", 7), ("pendulum", 8), ("cartpole", 8)])
def test_other_models(model, T):
    """nav2d (two steps per group), pendulum (one control: T = 7 leaves a ragged last group, T = 8 does not) and the cart-pole,
    whose lanes are redone with the library math when a fast path leaves its range."""
    check(lambda: make(model, T, N_RAGGED, 1.0))


def test_rider_block_of_a_lazy_state_sequence():
    """lazy_state_seq: the previous solve's state sequence rides in one extra block of the rollout launch, which takes no part
    in the sample loop; three solves."""
    check(lambda: make("racing", 8, N_RAGGED, 1.0, lazy_state_seq=True), steps=3)


def test_stamped_launch():
    check(lambda: make("racing", 8, N_RAGGED, 1.0), timing=2)
