"""2-D navigation among MOVING obstacles: Navigation2DEnv plus up to 8 discs with a constant-velocity prediction.

An occupancy grid has no time axis.  A pedestrian or another robot that will be somewhere else at step 20 of the horizon
has to be tested at step t against where it is predicted to be at step t: the cost reads a table with one row per horizon
step, `table[t, j] = (cx, cy, r2, w)` — centre, SQUARED radius and penalty of disc j at step t — and adds w for every
disc the position lies in (squared distance <= r2).  Overlapping discs add up.  `dynamics` / `cost_function` are tagged
"nav2d_discs", so MPPI runs them fused on the device (include/mppi_hip.h, mppi_set_discs, states the arithmetic); they are
plain torch in the same operation order and run anywhere, and behind untagged lambdas they take the generic path and mean
the same thing.

The terminal cost is evaluated with the stale info["t"] = T-1 (the reference's rule, src/pi_mpc/mppi.py:318-328), so it
reads row T-1: there is no row T.

The library holds no predictor: this class builds the table (constant velocity) and any other prediction can be written into
it.  The table is ONE tensor updated in place, so a captured graph of the callables (graph_callables=True) stays valid.
"""
from __future__ import annotations

from typing import Tuple

import torch

from envs.discs import MAX_DISCS, check_softness, disc_hits, disc_penalty, soft_coefficients, soft_disc_penalty
from envs.navigation_2d import Navigation2DEnv, _nav_inputs
from pi_mpc.native import native_model


def _moving_inputs(env: "MovingObstacleNav2DEnv") -> dict:
    spec = dict(_nav_inputs(env))
    spec["discs"] = {"table": env._disc_table, "version": env._disc_version}
    return spec


class MovingObstacleNav2DEnv(Navigation2DEnv):
    def __init__(self, horizon: int, device=torch.device("cuda"), dtype=torch.float32, seed: int = 42,
                 native_step: bool = True) -> None:
        """`horizon`: rows of the predicted table = the solver's horizon T."""
        if int(horizon) < 1:
            raise ValueError("horizon must be >= 1")
        super().__init__(device=device, dtype=dtype, seed=seed, native_step=native_step)
        self.horizon = int(horizon)
        self._disc_version = 0
        self._steps = torch.arange(self.horizon, device=self._device, dtype=dtype).view(-1, 1, 1) * self.delta_t  # t * delta_t
        self.set_moving_obstacles(torch.zeros(0, 2), torch.zeros(0, 2), 0.0)

    # ------------------------------------------------------------------ the obstacles
    def set_moving_obstacles(self, pos, vel, radius, weight=None) -> None:
        """pos [K, 2], vel [K, 2] (m, m/s), radius (float or [K], m), weight (float or [K]; None: obstacle_weight).
        K = 0 clears the obstacles; K > 8 raises ValueError."""
        kw = dict(device=self._device, dtype=self._dtype)
        pos = torch.as_tensor(pos, **kw).reshape(-1, 2).clone()
        vel = torch.as_tensor(vel, **kw).reshape(-1, 2).clone()
        K = pos.shape[0]
        if K > MAX_DISCS:
            raise ValueError(f"{K} moving obstacles: at most {MAX_DISCS}")
        if vel.shape[0] != K:
            raise ValueError("pos and vel must have one row per obstacle")
        radius = torch.as_tensor(radius, **kw).expand(K).clone() if K else torch.zeros(0, **kw)
        weight = self.obstacle_weight if weight is None else weight
        weight = torch.as_tensor(weight, **kw).expand(K).clone() if K else torch.zeros(0, **kw)
        if K and (not bool(torch.isfinite(pos).all() and torch.isfinite(vel).all() and torch.isfinite(radius).all()
                           and torch.isfinite(weight).all()) or bool((radius < 0).any()) or bool((weight < 0).any())):
            raise ValueError("moving obstacles: finite values, radius >= 0 and weight >= 0")
        self._disc_pos, self._disc_vel, self._disc_radius, self._disc_weight = pos, vel, radius, weight
        self._disc_table = torch.zeros(self.horizon, K, 4, **kw)  # (a new tensor only when the obstacle SET changes)
        self.predict_discs()

    def predict_discs(self) -> torch.Tensor:
        """The table [horizon, K, 4]: centres pos + vel * (t * delta_t) in fp32, r2 = radius * radius, the weights;
        written IN PLACE into one tensor.  Bumps the version the solver watches."""
        tab = self._disc_table
        if tab.shape[1]:
            tab[:, :, 0:2] = self._disc_pos.unsqueeze(0) + self._disc_vel.unsqueeze(0) * self._steps
            tab[:, :, 2] = (self._disc_radius * self._disc_radius).unsqueeze(0)
            tab[:, :, 3] = self._disc_weight.unsqueeze(0)
        self._disc_version += 1
        return tab

    def step(self, u: torch.Tensor) -> Tuple[torch.Tensor, bool]:
        out = super().step(u)  # (the parent's step: NativeStep("nav2d", ...) on a GPU — the discs are cost only)
        if self._disc_pos.shape[0]:
            self._disc_pos += self._disc_vel * self.delta_t
        self.predict_discs()
        return out

    # ------------------------------------------------------------------ the plugins
    @native_model("nav2d_discs", "dynamics", _moving_inputs)
    def dynamics(self, state: torch.Tensor, action: torch.Tensor, delta_t: float = 0.1) -> torch.Tensor:
        return Navigation2DEnv.dynamics(self, state, action, delta_t)

    @native_model("nav2d_discs", "cost", _moving_inputs)
    def cost_function(self, state: torch.Tensor, action: torch.Tensor, info: dict) -> torch.Tensor:
        # the parent's cost with the goal distance spelled out operation by operation, as the device forms it: two products,
        # one add, and the CORRECTLY ROUNDED square root (torch's vectorised fp32 sqrt on a CPU is a last bit off on 0.6 % of
        # the inputs; the root of an fp32 value taken in double and rounded once is exact)
        x, y = state[:, 0], state[:, 1]
        gx, gy = x - self._goal_pos[0], y - self._goal_pos[1]
        goal_cost = torch.sqrt((gx * gx + gy * gy).double()).to(state.dtype)
        occ = self._obstacle_map.compute_cost(state[:, :2].unsqueeze(1)).squeeze(1)
        base = goal_cost + self.obstacle_weight * occ
        return base + disc_penalty(self._disc_table[info["t"]], x, y)  # the discs where they are predicted to be at this step

    def collision_check(self, state: torch.Tensor) -> torch.Tensor:
        """The parent's static-map test plus the discs where they are NOW (row 0); > 0 means in collision."""
        hit = super().collision_check(state)
        return hit + disc_hits(self._disc_table[0], state).to(hit.dtype).reshape(hit.shape)


def _soft_moving_inputs(env: "SoftMovingObstacleNav2DEnv") -> dict:
    spec = dict(_moving_inputs(env))
    spec["discs"] = dict(spec["discs"], soft={"reach": env.soft_reach, "skirt": env.soft_skirt})
    return spec


class SoftMovingObstacleNav2DEnv(MovingObstacleNav2DEnv):
    """MovingObstacleNav2DEnv with a graded penalty SKIRT round every disc instead of the bare indicator: w inside a disc as
    before, outside it a ramp, linear in the squared distance, from `soft_skirt` * w at the rim to 0 at `soft_reach` * radius
    (include/mppi_hip.h, mppi_set_disc_softness, states the arithmetic) — so that a sample that keeps its distance is cheaper
    than one that grazes a rim.  One (reach, skirt) for all discs.  Tagged "nav2d_discs_soft"; every radius must be > 0.
    collision_check stays the hard test."""

    def __init__(self, horizon: int, soft_reach: float = 2.0, soft_skirt: float = 1.0, device=torch.device("cuda"),
                 dtype=torch.float32, seed: int = 42, native_step: bool = True) -> None:
        self.set_softness(soft_reach, soft_skirt)
        super().__init__(horizon, device=device, dtype=dtype, seed=seed, native_step=native_step)

    def set_softness(self, reach: float, skirt: float) -> None:
        """reach finite and > 1, skirt in [0, 1] (ValueError otherwise); takes effect with the next solve."""
        self._soft_reach, self._soft_skirt = check_softness(reach, skirt)
        self._soft_ab = soft_coefficients(self._soft_reach, self._soft_skirt)

    @property
    def soft_reach(self) -> float:
        return self._soft_reach

    @property
    def soft_skirt(self) -> float:
        return self._soft_skirt

    def set_moving_obstacles(self, pos, vel, radius, weight=None) -> None:
        """As the parent's, and every radius > 0 (the ramp divides by the squared radius)."""
        r = torch.as_tensor(radius, dtype=torch.float64)
        if torch.as_tensor(pos).numel() and not bool((r > 0).all()):
            raise ValueError("soft moving obstacles: every radius must be > 0")
        super().set_moving_obstacles(pos, vel, radius, weight)

    @native_model("nav2d_discs_soft", "dynamics", _soft_moving_inputs)
    def dynamics(self, state: torch.Tensor, action: torch.Tensor, delta_t: float = 0.1) -> torch.Tensor:
        return Navigation2DEnv.dynamics(self, state, action, delta_t)

    @native_model("nav2d_discs_soft", "cost", _soft_moving_inputs)
    def cost_function(self, state: torch.Tensor, action: torch.Tensor, info: dict) -> torch.Tensor:
        # the parent's base cost, operation by operation (see MovingObstacleNav2DEnv.cost_function), then the soft penalty
        x, y = state[:, 0], state[:, 1]
        gx, gy = x - self._goal_pos[0], y - self._goal_pos[1]
        goal_cost = torch.sqrt((gx * gx + gy * gy).double()).to(state.dtype)
        occ = self._obstacle_map.compute_cost(state[:, :2].unsqueeze(1)).squeeze(1)
        base = goal_cost + self.obstacle_weight * occ
        return base + soft_disc_penalty(self._disc_table[info["t"]], x, y, *self._soft_ab)
