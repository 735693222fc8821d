"""The regenerating horizon loop of trajectory_cost (csrc/mppi_rollout.hpp) walks only the groups that still have a successor
to generate, (T - 1) / SPG of them; the last group of the horizon, complete or ragged, goes through the epilogue, which
generates nothing.  On a real MI355X.  The tile-mode loop (`noise_regen` = 0) keeps its bound of T / SPG and is the in-tree
reference: costs, action sequence and state sequence of `noise_regen` = 1 must equal it bit for bit on a pair of handles with
equal seeds, over two solves of which the second is warm-started.

Shapes: the smallest at which the moved group can go wrong, at N = 64 (one wave) and N = 8192 + 37 (a last tile partly past
the end).  Four steps per group (pendulum): T = 4 is an empty loop with the whole horizon in the epilogue, T = 8 and 12 move
the last complete group there, T = 1, 2, 3 and 5, 9 keep their ragged last group.  Two steps per group (racing, nav2d): even
horizons move, T = 2 is the empty loop.  The cart-pole (per-lane redo with the library math) does NOT take the new bound: with
it 478 / 590 of 8 229 costs differed from tile mode at T = 4 / 8, because the compiler contracts its stage cost differently in
the loop and in the epilogue (profiles/r13_rollout_last_group.md); its cases hold the bound it keeps.  A start
outside the position clamp takes the copy whose `t == 0` test now runs in the epilogue (T = 1, 2) or in the loop (T = 3).  An
exploration fraction hands some lanes the all-zero mean copy.  The single-launch solve shares the loop (always regenerating):
a default solver is held to a multi-kernel tile-mode twin in `_costs` and the minimum.
"""
import pytest
import torch

from test_gpu_covariance import make
from test_gpu_fused_geometry import took
from test_gpu_rollout_drain import N_RAGGED, check

pytestmark = pytest.mark.gpu

SIZES = [64, N_RAGGED]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8, 9, 12])
def test_four_steps_per_group(T, N):
    check(lambda: make("pendulum", T, N, 1.0))


@pytest.mark.parametrize("T", [4, 8])
def test_redo_path(T):
    """cart-pole: lanes that leave a fast path's range are walked again with the library math, over the same bounds (the
    bound of every complete group: this model's epilogue is not bit-equal to its loop, see the module's docstring)."""
    check(lambda: make("cartpole", T, N_RAGGED, 1.0))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("T", [6, 10])
def test_two_steps_per_group_racing(T, N):
    check(lambda: make("racing", T, N, 1.0))


def test_two_steps_per_group_empty_loop():
    check(lambda: make("nav2d", 2, N_RAGGED, 1.0))


@pytest.mark.parametrize("T", [1, 2, 3])
def test_start_outside_the_position_clamp(T):
    def build():
        solver, x0 = make("racing", T, N_RAGGED, 1.0)
        x0 = x0.clone()
        x0[0] = 41.5  # (the map spans +-40 m)
        return solver, x0
    check(build)


@pytest.mark.parametrize("model", ["pendulum", "racing"])
def test_exploration_split(model):
    """The lanes past the exploration threshold read the all-zero copy of the mean, also in the epilogue."""
    check(lambda: make(model, 8, N_RAGGED, 1.0, exploration=0.3))


@pytest.mark.parametrize("N", [64, 4096])
@pytest.mark.parametrize("T", [2, 4, 8])
@pytest.mark.parametrize("model", ["racing", "pendulum"])
def test_single_launch(model, T, N):
    """A default solver (one cooperative launch, regenerating loop) against an equal-seed twin on the multi-kernel path in
    tile mode; the twin is fed the same warm start before the second solve."""
    fused, x0 = make(model, T, N, 1.0)
    tiles, _ = make(model, T, N, 1.0)
    tiles.set_option("fused_solve", 0)
    tiles.set_option("noise_regen", 0)
    assert fused._one_call and tiles._one_call
    x = x0.cuda()
    for k in range(2):
        name = f"{model} T{T} N{N} solve {k}"
        if k:
            tiles.set_warm_start(fused._previous_action_seq.cpu().numpy())
        a, s = fused.forward(x)
        tiles.forward(x)
        assert took(fused._h) != (0, 0), f"{name}: the default solver did not take the single launch"
        assert took(tiles._h) == (0, 0), name
        assert torch.isfinite(tiles._costs).all() and torch.isfinite(a).all() and torch.isfinite(torch.as_tensor(s)).all(), name
        assert torch.equal(fused._costs, tiles._costs), (name, int((fused._costs != tiles._costs).sum()))
        assert fused.last_stats()["cmin"] == tiles.last_stats()["cmin"] == float(tiles._costs.min()), name
