"""The moving-disc rule in torch, once.  A row [K, 4] holds (cx, cy, r2, w) per slot; a position is in disc j when its squared
distance to the centre is <= r2; overlapping discs add up (include/mppi_hip.h, mppi_set_discs: the device's arithmetic)."""
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


def disc_hits(row: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """How many discs of `row` each position of state [..., >= 2] lies in."""
    hit = torch.zeros(state.shape[:-1], device=state.device, dtype=state.dtype)
    for j in range(row.shape[0]):
        dx, dy = state[..., 0] - row[j, 0], state[..., 1] - row[j, 1]
        hit = hit + ((dx * dx + dy * dy) <= row[j, 2]).to(hit.dtype)
    return hit
