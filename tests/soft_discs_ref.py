"""numpy restatement of the SOFT moving-disc rule for both disc models (MPPI_MODEL_NAV2D_DISCS_SOFT / MPPI_MODEL_RACING_DISCS_SOFT:
csrc/mppi_models.inc, csrc/mppi_discs.hpp; include/mppi_hip.h, mppi_set_disc_softness, states the rule) for the CPU and the
GPU tests.  Steps, base costs, the `near` / `edge` boundary rule, cap(N) and the case tables are those of discs_ref.py and
racing_discs_ref.py, unchanged; only the row penalty is new:

    inside the disc (the hard rule's own compare, d2 <= r2) the penalty is w; outside it is w * max(a - b * d2 / r2, 0),
    a = fl32(phi k / (k - 1)), b = fl32(phi / (k - 1)), k = reach^2, phi = skirt, each formed in double and rounded once.

  fp32, fuse=False (math level 0): every operation rounded on its own, IEEE quotient.
  fp32, fuse=True (the fast levels): d2 = fma(dx, dx, dy*dy), q = d2 * (1 / r2), ramp = max(fma(-b, q, a), 0), pen = fma(w, f, pen),
    each fma rounded ONCE (fma32 below), the reciprocal the IEEE quotient a host build forms (the device's is 1 ulp off).
  float64: the yardstick of the fast levels, with the SAME two fp32 coefficients.
`wrong` selects a misreading of the rule the tests must be able to tell apart (test_the_restatement_can_fail).
The penalty is continuous at the rim for skirt = 1 and jumps by (1 - skirt) w there otherwise; it is continuous where the skirt
ends (the max with 0).  So the `near` rule of the hard models (|dist - r| <= 1e-4 m) is the only boundary the fast levels need.

The float64 yardstick is evaluated ON THE SAME STATES as the fp32 costs it judges (rollout_*(..., dtype=f64, states=S)).  The hard
indicator is flat away from a rim, so a position that is one fp32 rounding off (1e-6 m at 9 m from the origin) changes no cost
outside the `near` band, and the hard models' tests can compare against a float64 rollout of its own.  A ramp is not flat: its
slope is up to 2 w b reach / r per metre (500 per metre for w = 30, r = 0.25 m, reach = 1.25), which turns that 1e-6 m into
5e-4 per step — measured on these tables: up to 1.3e-5 (nav2d) and 5.4e-6 (racing) of the cost scale between the fp32 and the
float64 rollout, each on its own states, against 3.1e-7 and 2.2e-7 on the same states.  The first figure is a property of fp32
states under any graded cost, not of the arithmetic under test; the dynamics are the hard models' own, unchanged, and their
tests hold them.
"""
import numpy as np

import discs_ref as D
import racing_discs_ref as RD
from discs_ref import MAX_DISCS, NEAR_M, EDGE_CELLS, PARITY, cap  # noqa: F401  (one owner each)

f32, f64 = np.float32, np.float64
SETTINGS = ((1.25, 1.0), (2.0, 1.0), (2.0, 0.25), (3.0, 0.5))  # (reach, skirt)
HARD = (2.0, 0.0)                                              # skirt = 0: a = b = 0, the hard rule's bits
SAMPLES, HORIZONS, T_LONG = D.SAMPLES, D.HORIZONS, D.T_LONG
ALL_T = HORIZONS + (T_LONG,)
assert set(RD.HORIZONS) == set(ALL_T) and RD.SAMPLES == SAMPLES
WRONG = ("ramp_in_d", "skirt_inside", "swapped")


def coefficients(reach, skirt):
    """-> (a, b) as the library forms them: the fp32 arguments, the arithmetic in double, each result rounded once"""
    kappa, phi = float(f32(reach)) * float(f32(reach)), float(f32(skirt))
    return f32(phi * kappa / (kappa - 1.0)), f32(phi / (kappa - 1.0))


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for fp32 arrays: the product of two fp32 values is exact in double; the sum with c
    is formed with its exact error (TwoSum) and rounded to odd, and a 53-bit round-to-odd value rounds to 24 bits as the exact
    sum does."""
    p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
    c = np.broadcast_to(np.asarray(c, f32).astype(f64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    with np.errstate(invalid="ignore"):
        fix = (err != 0) & np.isfinite(s) & ((s.view(np.int64) & 1) == 0)
        other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where(fix, other, s).astype(f32)


def soft_penalty(row, n, x, y, a, b, dtype=f32, fuse=False, wrong=None, reach=None, skirt=None):
    """-> (pen [N], hit [N, n], skirted [N, n]): the discs 0 .. n-1 of one row [>= n, 4], in slot order.  hit: inside the disc;
    skirted: outside it with 0 < ramp.  a, b: the two fp32 coefficients.  `wrong` (fp32 level 0 only) needs reach and skirt."""
    row = np.asarray(row, f32).astype(dtype)
    a, b = dtype(f32(a)), dtype(f32(b))
    if wrong == "swapped":
        a, b = b, a
    pen = np.zeros(x.shape[0], dtype)
    hit = np.zeros((x.shape[0], n), bool)
    skirted = np.zeros((x.shape[0], n), bool)
    zero, one = dtype(0.0), dtype(1.0)
    for j in range(n):
        dx, dy = x - row[j, 0], y - row[j, 1]
        r2, w = row[j, 2], row[j, 3]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if fuse and dtype == f32:
                d2 = fma32(dx, dx, dy * dy)
                q = d2 * (one / r2)
                ramp = np.fmax(fma32(-b, q, a), zero)
            else:
                d2 = dx * dx + dy * dy
                q = d2 / r2
                ramp = np.fmax(a - b * q, zero)
            if wrong == "ramp_in_d":  # linear in the distance, from skirt * w at the rim to 0 at reach * r
                ramp = np.fmax(dtype(skirt) * (dtype(reach) - np.sqrt(q)) / dtype(reach - 1.0), zero).astype(dtype)
        hit[:, j] = d2 <= r2
        inside = dtype(skirt) if wrong == "skirt_inside" else one
        f = np.where(hit[:, j], inside, ramp).astype(dtype)
        skirted[:, j] = ~hit[:, j] & (ramp > 0)
        pen = fma32(w, f, pen) if fuse and dtype == f32 else (pen + w * f).astype(dtype)
    return pen, hit, skirted


def _boundaries(row, n, s, grids, near, edge):
    """the boundary rule of discs_ref.py / racing_discs_ref.py on float64 states: `near` a rim, `edge` of a map cell"""
    for j in range(n):
        d = np.sqrt((s[:, 0] - f64(row[j, 0])) ** 2 + (s[:, 1] - f64(row[j, 1])) ** 2)
        if row[j, 2] >= 0:
            near |= np.abs(d - np.sqrt(f64(row[j, 2]))) <= NEAR_M
    e = EDGE_CELLS * grids[0][1]
    occ = (lambda x, y: D.occupancy(grids[0], x, y, f64)) if len(grids) == 1 else (lambda x, y: RD.occupancy2(grids, x, y, f64))
    o = occ(s[:, 0], s[:, 1])
    for ex, ey in ((e, e), (e, -e), (-e, e), (-e, -e)):
        edge |= occ(s[:, 0] + ex, s[:, 1] + ey) != o


def rollout_nav2d(P, grid, table, x0, U, a, b, dtype=f32, states=None, fuse=False, **kw):
    """discs_ref.rollout with the soft row penalty -> dict(costs, S, hit, skirted, near, edge, scale)"""
    U = np.asarray(U)
    N, T, _ = U.shape
    table = np.asarray(table, f32)
    n = table.shape[1]
    assert table.shape[0] >= T and n <= MAX_DISCS
    Ud = U.astype(dtype)
    s = np.broadcast_to(np.asarray(x0, f32).astype(dtype), (N, 3)).copy()
    S = np.empty((N, T + 1, 3), dtype)
    H, K = np.zeros((N, T + 1, n), bool), np.zeros((N, T + 1, n), bool)
    acc = np.zeros(N, f64)
    near, edge = np.zeros(N, bool), np.zeros(N, bool)
    for t in range(T + 1):
        if states is not None:
            s = np.asarray(states[:, t], f32).astype(dtype)
        S[:, t] = s
        row = table[min(t, T - 1)]
        pen, H[:, t], K[:, t] = soft_penalty(row, n, s[:, 0], s[:, 1], a, b, dtype, fuse, **kw)
        c = (D.base_cost(P, grid, s, dtype) + pen).astype(dtype)
        acc += c.astype(f64)  # (CostSum<true>: added in double, rounded once)
        if dtype == f64:
            _boundaries(row, n, s, (grid,), near, edge)
        if t < T and states is None:
            s = D.step(P, s, Ud[:, t], dtype)
    costs = acc.astype(f32) if dtype == f32 else acc
    return dict(costs=costs, S=S, hit=H, skirted=K, near=near, edge=edge, scale=float(np.max(np.abs(acc))))


def rollout_racing(P, grids, ref, table, x0, U, a, b, dtype=f32, states=None, fuse=False, **kw):
    """racing_discs_ref.rollout with the soft row penalty (sequential cost sum in the working precision)"""
    U = np.asarray(U)
    N, T, _ = U.shape
    table = np.asarray(table, f32)
    n = table.shape[1]
    Kr = RD.ref_rows(ref, dtype)
    assert table.shape[0] >= T and Kr.shape[0] >= T and n <= MAX_DISCS
    Ud = U.astype(dtype)
    s = np.broadcast_to(np.asarray(x0, f32).astype(dtype), (N, 4)).copy()
    S = np.empty((N, T + 1, 4), dtype)
    H, K = np.zeros((N, T + 1, n), bool), np.zeros((N, T + 1, n), bool)
    acc = np.zeros(N, dtype)
    near, edge = np.zeros(N, bool), np.zeros(N, bool)
    zero = np.zeros((N, 2), dtype)
    for t in range(T + 1):
        if states is not None:
            s = np.asarray(states[:, t], f32).astype(dtype)
        S[:, t] = s
        row = min(t, T - 1)
        u = Ud[:, t] if t < T else zero
        pu = Ud[:, max(t - 1, 0)] if t < T else Ud[:, max(T - 2, 0)]
        pen, H[:, t], K[:, t] = soft_penalty(table[row], n, s[:, 0], s[:, 1], a, b, dtype, fuse, **kw)
        c = (RD.base_cost(P, grids, Kr[row], s, u, pu, dtype) + pen).astype(dtype)
        acc = (acc + c).astype(dtype)
        if dtype == f64:
            _boundaries(table[row], n, s, grids, near, edge)
        if t < T and states is None:
            s = RD.step(P, s, Ud[:, t], dtype)
    return dict(costs=acc, S=S, hit=H, skirted=K, near=near, edge=edge, scale=float(np.max(np.abs(acc.astype(f64)))))
