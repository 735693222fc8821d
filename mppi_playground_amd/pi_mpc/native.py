"""Plugin recognition: how a `dynamics` / `cost_func` callable tells the solver that it is one of the
shipped models and can run fused on the device.

The reference's plugin surface is two opaque Python callables (src/pi_mpc/mppi.py:30-31,55-56).  The
call site `MPPI(..., dynamics=env.dynamics, cost_func=ctrl.cost_function)` stays unchanged: a callable
(or the function object behind a bound method) carries an attribute

    __mppi_native__ = NativeTag(model, role, provider)

where `provider(owner)` returns the model's current inputs as plain host data:
    {"params": [floats], "maps": [GridSpec, ...], "ref_path": ndarray[rows,4] | None,
     "mlp": {"table": float32[n], "hidden_layers": 1 | 2, "activation": "relu" | "tanh", "residual": bool, "version": int,
             "value": None | {"table": float32[32 * DS + 1121], "hidden_layers": 1 | 2, "activation": ..., "weight": float,
                              "replace_terminal": bool, "version": int}   (the learned terminal value: uploaded by version, and
                              only by a solver that was given the model's callable of role "terminal" as `terminal_cost`)},
     "discs": {"table": float32 [rows, n, 4] = {cx, cy, r2, w} per horizon step (a torch tensor on the solver's device, or
               an ndarray), "version": int,
               "soft": {"reach": float > 1, "skirt": float in [0, 1]}  (the soft disc models only)}}
("mlp": the learned-dynamics models only — an ensemble (envs.MLPEnsemble) adds "tables": float32 [E, n] (row e: member e's
table), "nominal": the member "table" is, and "member_versions": one version per member, so that the solver re-uploads only the
members that changed; "discs": the moving-disc models only — "nav2d_discs" (envs.MovingObstacleNav2DEnv)
and "racing_discs" (envs.racing_opponents: opponent cars, next to racing's "ref_path" or device-built window) — rows >= the
horizon and n <= 8 or the solver raises ValueError; either table is uploaded again when its `version` changes.  "soft": the
graded skirt of "nav2d_discs_soft" / "racing_discs_soft" (envs.SoftMovingObstacleNav2DEnv, envs.racing_opponents'
Soft classes); the solver hands the pair to mppi_set_disc_softness before a solve whenever it changed.)
`owner` is the bound method's `__self__` (None for plain functions).  The solver calls the provider
of the cost callable before every solve (the racing reference window changes every tick,
example/racing.py:73-81) and re-uploads only what changed.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np


@dataclass(frozen=True)
class NativeTag:
    model: object                 # a key of _capi.MODEL_IDS ("pendulum", "racing", ...), or model(owner) -> such a key
                                  # (resolve() calls it: envs/mlp_model.py picks "mlp41" / "mlp42" / "mlp81" / ... by its widths)
    role: str                     # "dynamics" | "cost" | "terminal" (MPPI(terminal_cost=): envs.MLPModel.terminal_cost)
    provider: Optional[Callable]  # provider(owner) -> dict
    per_owner: bool = False       # the model name came from the owner (below): dynamics and cost must share ONE owner


@dataclass
class GridSpec:
    cells: np.ndarray   # uint8 [nx][ny] occupancy (0/1)
    cell_size: float
    origin: tuple       # (ox, oy) cell index of world (0, 0)
    version: int = 0    # bump when cells change
    # optional integer description the solver can rasterise on the device instead of uploading `cells`:
    #   {"kind": "obstacles", "circles": int32[nc,3] (ci, cj, r cells), "rects": int32[nr,4] (x0, x1, y0, y1)}
    #   {"kind": "lane", "seeds": int32[ns,2], "max_d2": int}
    recipe: Optional[dict] = None


def native_model(model: str, role: str, provider: Optional[Callable] = None):
    """Decorator: tag a function / method as the native `role` of `model`."""

    def deco(fn):
        fn.__mppi_native__ = NativeTag(model, role, provider)
        return fn

    return deco


def resolve(fn):
    """-> (NativeTag, owner) or None.  Works for plain functions, bound methods, callable objects."""
    tag = getattr(fn, "__mppi_native__", None)
    if tag is None and hasattr(fn, "__func__"):
        tag = getattr(fn.__func__, "__mppi_native__", None)
    if not isinstance(tag, NativeTag):
        return None
    owner = getattr(fn, "__self__", None)
    if callable(tag.model):
        tag = NativeTag(tag.model(owner), tag.role, tag.provider, True)
    return tag, owner
