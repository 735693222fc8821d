"""The moving-disc rule in torch, once.  A row [K, 4] holds (cx, cy, r2, w) per slot; a position is in disc j when its squared
distance to the centre is <= r2; overlapping discs add up (include/mppi_hip.h, mppi_set_discs: the device's arithmetic).
The soft rule (mppi_set_disc_softness) adds a graded skirt outside the disc: soft_coefficients / soft_disc_penalty."""
import math

import numpy as np
import torch

from mppi_playground_amd._capi import MAX_DISCS  # noqa: F401  (MPPI_MAX_DISCS: the envs take it from here)


def disc_penalty(row: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Sum of w over the discs of `row` that (x, y) lies in, in the device's operation order."""
    pen = torch.zeros_like(x)
    for j in range(row.shape[0]):
        dx, dy = x - row[j, 0], y - row[j, 1]
        d2 = dx * dx + dy * dy
        pen = pen + torch.where(d2 <= row[j, 2], row[j, 3], torch.zeros_like(x))
    return pen


def check_softness(reach, skirt) -> tuple:
    """(reach, skirt) of the soft disc models as floats, or ValueError: reach finite and > 1, skirt in [0, 1]
    (include/mppi_hip.h, mppi_set_disc_softness)."""
    reach, skirt = float(reach), float(skirt)
    if not (math.isfinite(reach) and reach > 1.0 and 0.0 <= skirt <= 1.0):
        raise ValueError(f"disc softness: reach finite and > 1, skirt in [0, 1]; got reach={reach}, skirt={skirt}")
    return reach, skirt


def soft_coefficients(reach, skirt) -> tuple:
    """-> (a, b), the two fp32 coefficients of the soft rule as the library forms them: with k = reach^2 (of the fp32 values),
    a = fl32(skirt * k / (k - 1)), b = fl32(skirt / (k - 1)), the arithmetic in double, each result rounded once."""
    kappa, phi = float(np.float32(reach)) * float(np.float32(reach)), float(np.float32(skirt))
    return float(np.float32(phi * kappa / (kappa - 1.0))), float(np.float32(phi / (kappa - 1.0)))


def soft_disc_penalty(row: torch.Tensor, x: torch.Tensor, y: torch.Tensor, a: float, b: float) -> torch.Tensor:
    """The soft rule in the device's level-0 operation order: w inside a disc (the hard rule's own compare), outside it
    w * max(a - b * d2 / r2, 0) — linear in d2 from skirt * w at the rim to 0 at reach * r.  Every r2 of `row` must be > 0."""
    pen = torch.zeros_like(x)
    for j in range(row.shape[0]):
        dx, dy = x - row[j, 0], y - row[j, 1]
        d2 = dx * dx + dy * dy
        q = d2 / row[j, 2]
        ramp = torch.clamp(a - b * q, min=0.0)
        pen = pen + row[j, 3] * torch.where(d2 <= row[j, 2], torch.ones_like(x), ramp)
    return pen


def disc_hits(row: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """How many discs of `row` each position of state [..., >= 2] lies in."""
    hit = torch.zeros(state.shape[:-1], device=state.device, dtype=state.dtype)
    for j in range(row.shape[0]):
        dx, dy = state[..., 0] - row[j, 0], state[..., 1] - row[j, 1]
        hit = hit + ((dx * dx + dy * dy) <= row[j, 2]).to(hit.dtype)
    return hit
