"""Racing among OPPONENT CARS: RacingEnv / racing_controller plus up to 8 moving discs, one table row per horizon step.

The racing track is an occupancy grid and has no time axis.  A slower car ahead has to be tested at step t of a sample
against where that car will be at step t: the cost reads a table `table[t, j] = (cx, cy, r2, w)` — centre, SQUARED radius
and penalty of car j at step t — and adds w for every disc the position lies in (squared distance <= r2), after racing's
own cost.  `OpponentRacingEnv.dynamics` and `opponent_racing_controller.cost_function` are tagged "racing_discs", so MPPI
runs them fused on the device (include/mppi_hip.h, mppi_set_discs, states the arithmetic); they are plain torch in the same
operation order and run anywhere, and behind untagged lambdas they take the generic path and mean the same thing.

The terminal cost is evaluated with the stale info["t"] = T-1 (the reference's rule, src/pi_mpc/mppi.py:318-328), so it
reads reference row and disc row T-1: there is no row T.

The library holds no predictor: the env builds the table (each car follows the centre line at its own constant speed,
optionally offset sideways) and any other prediction can be written into it.  The table is ONE tensor updated in place.
The cars do not react to the ego car.
"""
from __future__ import annotations

from typing import Tuple

import torch

from envs.discs import MAX_DISCS, check_softness, disc_hits, disc_penalty, soft_coefficients, soft_disc_penalty
from envs.racing_controller import _racing_cost_inputs, racing_controller
from envs.racing_env import RacingEnv, _racing_dyn_inputs
from pi_mpc.native import native_model


class OpponentRacingEnv(RacingEnv):
    def __init__(self, horizon: int = 25, device=torch.device("cuda"), dtype=torch.float32, seed: int = 42,
                 native_step: bool = True) -> None:
        """`horizon`: rows of the predicted table = the solver's horizon T."""
        if int(horizon) < 1:
            raise ValueError("horizon must be >= 1")
        super().__init__(device=device, dtype=dtype, seed=seed, native_step=native_step)
        self.horizon = int(horizon)
        self.opponent_weight = 10000.0  # racing_controller's obstacle weight Qo: a car costs what a wall costs
        yaw = self.racing_center_path[:, 2]
        self._center_normal = torch.stack([-torch.sin(yaw), torch.cos(yaw)], dim=1)  # left normal of the centre line
        # arc length travelled by step t of the horizon per unit speed, in float64: the path index is an exact statement
        self._steps = torch.arange(self.horizon, device=self._device, dtype=torch.float64).view(-1, 1) * self.delta_t
        self._opp_version = 0
        self.set_opponents([], [], 0.0)

    # ------------------------------------------------------------------ the cars
    def set_opponents(self, path_index, speed, radius, lateral_offset=0.0, weight=None) -> None:
        """path_index [K] (index into racing_center_path where car j is now), speed [K] (m/s along the centre line),
        radius (float or [K], m), lateral_offset (float or [K], m along the path's left normal), weight (float or [K];
        None: opponent_weight).  K = 0 clears the cars; K > 8 raises ValueError."""
        kw = dict(device=self._device, dtype=self._dtype)
        index = torch.as_tensor(path_index, device=self._device, dtype=torch.float64).reshape(-1).clone()
        K = index.shape[0]
        if K > MAX_DISCS:
            raise ValueError(f"{K} opponent cars: at most {MAX_DISCS}")
        speed = torch.as_tensor(speed, device=self._device, dtype=torch.float64).reshape(-1).clone()
        if speed.shape[0] != K:
            raise ValueError("path_index and speed must have one entry per car")
        weight = self.opponent_weight if weight is None else weight
        expand = lambda v: torch.as_tensor(v, **kw).expand(K).clone() if K else torch.zeros(0, **kw)  # noqa: E731
        radius, offset, weight = expand(radius), expand(lateral_offset), expand(weight)
        if K and (not bool(torch.isfinite(index).all() and torch.isfinite(speed).all() and torch.isfinite(radius).all()
                           and torch.isfinite(offset).all() and torch.isfinite(weight).all())
                  or bool((index < 0).any()) or bool((radius < 0).any()) or bool((weight < 0).any())):
            raise ValueError("opponent cars: finite values, path_index >= 0, radius >= 0 and weight >= 0")
        self._opp_s = index * self.dl  # arc position along the centre line, metres (float64)
        self._opp_speed, self._opp_radius, self._opp_offset, self._opp_weight = speed, radius, offset, weight
        self._opp_table = torch.zeros(self.horizon, K, 4, **kw)  # (a new tensor only when the SET of cars changes)
        self.predict_opponents()

    def opponent_path_indices(self) -> torch.Tensor:
        """[horizon, K] centre-line index of car j at step t: round((s_j + v_j * t * delta_t) / dl), half to even, held at the
        last point of the course."""
        idx = torch.round((self._opp_s.unsqueeze(0) + self._opp_speed.unsqueeze(0) * self._steps) / self.dl).long()
        return idx.clamp_(0, self.racing_center_path.shape[0] - 1)

    def predict_opponents(self) -> torch.Tensor:
        """The table [horizon, K, 4]: centre = centre-line point + lateral_offset * left normal at that point (fp32), r2 =
        radius * radius, the weights; written IN PLACE into one tensor.  Bumps the version the solver watches."""
        tab = self._opp_table
        if tab.shape[1]:
            idx = self.opponent_path_indices()
            tab[:, :, 0:2] = self.racing_center_path[idx][:, :, 0:2] + self._opp_offset.view(1, -1, 1) * self._center_normal[idx]
            tab[:, :, 2] = (self._opp_radius * self._opp_radius).unsqueeze(0)
            tab[:, :, 3] = self._opp_weight.unsqueeze(0)
        self._opp_version += 1
        return tab

    def step(self, u: torch.Tensor) -> Tuple[torch.Tensor, bool]:
        out = super().step(u)  # (the parent's step: NativeStep("racing", ...) on a GPU — the cars are cost only)
        if self._opp_s.shape[0]:
            self._opp_s += self._opp_speed * self.delta_t
        self.predict_opponents()
        return out

    # ------------------------------------------------------------------ the plugins
    @native_model("racing_discs", "dynamics", _racing_dyn_inputs)
    def dynamics(self, state: torch.Tensor, action: torch.Tensor, delta_t: float = 0.1) -> torch.Tensor:
        return RacingEnv.dynamics(self, state, action, delta_t)

    def opponent_hits(self, state: torch.Tensor) -> torch.Tensor:
        """How many cars, where they are NOW (row 0), each position of state [..., >= 2] lies in."""
        return disc_hits(self._opp_table[0], state)

    def collision_check(self, state: torch.Tensor) -> torch.Tensor:
        """The parent's static-map test plus the cars where they are NOW (row 0); > 0 means in collision."""
        hit = super().collision_check(state)
        return hit + self.opponent_hits(state).reshape(hit.shape)


def _opponent_cost_inputs(ctrl: "opponent_racing_controller") -> dict:
    spec = dict(_racing_cost_inputs(ctrl))
    spec["discs"] = {"table": ctrl.env._opp_table, "version": ctrl.env._opp_version}
    return spec


class opponent_racing_controller(racing_controller):
    """racing_controller over an OpponentRacingEnv: the same tick (reference window on the device), the cost with the cars."""

    @native_model("racing_discs", "cost", _opponent_cost_inputs)
    def cost_function(self, state: torch.Tensor, action: torch.Tensor, info: dict) -> torch.Tensor:
        base = racing_controller.cost_function(self, state, action, info)
        x, y = state[:, 0], state[:, 1]
        row = self.env._opp_table[info["t"]].to(state.device)  # [K, 4]: the cars where they are predicted to be at this step
        return base + disc_penalty(row, x, y)


class SoftOpponentRacingEnv(OpponentRacingEnv):
    """OpponentRacingEnv whose cars carry a graded penalty SKIRT (include/mppi_hip.h, mppi_set_disc_softness): w inside a car's
    disc as before, outside it a ramp, linear in the squared distance, from `soft_skirt` * w at the rim to 0 at `soft_reach` *
    radius.  One (reach, skirt) for all cars; every radius must be > 0.  The pair lives here; soft_opponent_racing_controller's
    cost reads it.  Tagged "racing_discs_soft"; collision_check stays the hard test."""

    def __init__(self, horizon: int = 25, soft_reach: float = 2.0, soft_skirt: float = 1.0, device=torch.device("cuda"),
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

    def set_opponents(self, path_index, speed, radius, lateral_offset=0.0, weight=None) -> None:
        """As the parent's, and every radius > 0 (the ramp divides by the squared radius)."""
        r = torch.as_tensor(radius, dtype=torch.float64)
        if torch.as_tensor(path_index).numel() and not bool((r > 0).all()):
            raise ValueError("soft opponent cars: every radius must be > 0")
        super().set_opponents(path_index, speed, radius, lateral_offset, weight)

    @native_model("racing_discs_soft", "dynamics", _racing_dyn_inputs)
    def dynamics(self, state: torch.Tensor, action: torch.Tensor, delta_t: float = 0.1) -> torch.Tensor:
        return RacingEnv.dynamics(self, state, action, delta_t)


def _soft_opponent_cost_inputs(ctrl: "soft_opponent_racing_controller") -> dict:
    spec = dict(_opponent_cost_inputs(ctrl))
    spec["discs"] = dict(spec["discs"], soft={"reach": ctrl.env.soft_reach, "skirt": ctrl.env.soft_skirt})
    return spec


class soft_opponent_racing_controller(opponent_racing_controller):
    """opponent_racing_controller over a SoftOpponentRacingEnv: the same tick, the cost with the cars' skirts."""

    @native_model("racing_discs_soft", "cost", _soft_opponent_cost_inputs)
    def cost_function(self, state: torch.Tensor, action: torch.Tensor, info: dict) -> torch.Tensor:
        base = racing_controller.cost_function(self, state, action, info)
        x, y = state[:, 0], state[:, 1]
        row = self.env._opp_table[info["t"]].to(state.device)  # [K, 4]: the cars where they are predicted to be at this step
        return base + soft_disc_penalty(row, x, y, *self.env._soft_ab)
