"""numpy restatement of the moving-disc model (MPPI_MODEL_NAV2D_DISCS: csrc/mppi_models.inc, csrc/mppi_discs.hpp;
include/mppi_hip.h, mppi_set_discs, states the rule) and the case table the CPU and the GPU tests share.

  step / cost / rollout in fp32 — every operation rounded on its own, in the order the header states, sin / cos / fmod from the
  C library the host build of the functor links (so the two agree bit for bit) — and in float64 (the yardstick of the fast levels).
  The stage cost of step t reads row t of the table, the terminal cost row T-1 (there is no row T).
  rollout(..., states=S) evaluates the costs on GIVEN states (a device's own: its sin / cos are another library's, every
  operation of the cost — subtract, multiply, add, sqrt, divide, round, compare — is exactly rounded everywhere).

Boundary rule of the fast levels: a sample is left out of a cost comparison when, in float64, some (t, j) has
|dist - r| <= 1e-4 m (`near`), or a map-cell rounding lies within 1e-3 cell of a cell of another value (`edge`: the parity
rule of test_gpu_parity.py).  cap(N) = max(2, 0.02 N) bounds how many `near` samples a case may leave out.
"""
import ctypes
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
MAX_DISCS, KROW = 8, 32
PAD = f32([0.0, 0.0, -1.0, 0.0])  # an unused slot of the padded table
PI_F, TWO_PI_F = f32(3.14159274), f32(6.28318548)
X0 = f32([-9.0, -9.0, 0.78539816])       # the start pose the discs are placed ahead of
X0_OUT = f32([-10.5, -9.0, 0.78539816])  # a start outside the position clamp (the X0OUT copy of the loop)
MEAN, SIGMAS, U_MIN, U_MAX = f32([1.0, 0.0]), f32([0.5, 0.5]), f32([0.0, -1.0]), f32([2.0, 1.0])
SAMPLES = (64, 100, 4160)        # one tile, a ragged tile, more than the single launch takes
HORIZONS = (1, 2, 3, 7, 8)       # dc = 2: the group loop, both drain halves, the ragged and the complete epilogue
T_LONG = 25
NEAR_M, EDGE_CELLS = 1e-4, 1e-3
PARITY = 2e-6                    # of the cost scale

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]
_sinf = np.frompyfunc(lambda v: _libm.sinf(float(v)), 1, 1)
_cosf = np.frompyfunc(lambda v: _libm.cosf(float(v)), 1, 1)


def cap(N):
    return max(2, int(0.02 * N))


def _trig(theta, dtype):
    if dtype == f32:
        return _sinf(theta).astype(f32), _cosf(theta).astype(f32)
    return np.sin(theta), np.cos(theta)


def angle_normalize(x, dtype):
    """((x + pi) % 2 pi) - pi with torch.remainder semantics (fmod + sign fix); fmod is exact in any library"""
    pi, two_pi = dtype(PI_F), dtype(TWO_PI_F)
    r = np.fmod(x + pi, two_pi)
    r = np.where((r != 0) & (r < 0), r + two_pi, r)
    return (r - pi).astype(dtype)


def step(P, s, u, dtype=f32):
    """Model<NAV2D>::step at math level 0: P = the 12 MPPI_NP_* parameters, s [N, 3], u [N, 2] -> next state [N, 3]"""
    P = np.asarray(P, f32).astype(dtype)
    v = np.clip(u[:, 0], P[0], P[1])
    om = np.clip(u[:, 1], P[2], P[3])
    th = angle_normalize(s[:, 2], dtype)
    sn, cs = _trig(th, dtype)
    nx = s[:, 0] + (v * cs) * P[4]
    ny = s[:, 1] + (v * sn) * P[4]
    nth = angle_normalize(th + om * P[4], dtype)
    return np.stack([np.clip(nx, P[5], P[6]), np.clip(ny, P[7], P[8]), nth], 1).astype(dtype)


def occupancy(grid, x, y, dtype=f32):
    """occ_lookup: idx = round_half_even(p / cell + origin); out of bounds -> 1"""
    cells, cell, ox, oy = grid
    qx = np.rint(x / dtype(f32(cell)) + dtype(f32(ox)))
    qy = np.rint(y / dtype(f32(cell)) + dtype(f32(oy)))
    ix, iy = qx.astype(np.int64), qy.astype(np.int64)
    inb = (ix >= 0) & (ix < cells.shape[0]) & (iy >= 0) & (iy < cells.shape[1])
    v = cells[np.clip(ix, 0, cells.shape[0] - 1), np.clip(iy, 0, cells.shape[1] - 1)].astype(dtype)
    return np.where(inb, v, dtype(1.0))


def base_cost(P, grid, s, dtype=f32):
    P = np.asarray(P, f32).astype(dtype)
    dx, dy = s[:, 0] - P[9], s[:, 1] - P[10]
    goal = np.sqrt(dx * dx + dy * dy)
    return (goal + P[11] * occupancy(grid, s[:, 0], s[:, 1], dtype)).astype(dtype)


def penalty(row, n, x, y, dtype=f32, fuse=False):
    """-> (pen [N], hit [N, n]): the discs 0 .. n-1 of one row [>= n, 4], in slot order.  fuse: d2 = fma(dx, dx, dy * dy)
    (the fast levels; fp32 only: the product-sum in float64, rounded once)."""
    row = np.asarray(row, f32).astype(dtype)
    pen = np.zeros(x.shape[0], dtype)
    hit = np.zeros((x.shape[0], n), bool)
    for j in range(n):
        dx, dy = x - row[j, 0], y - row[j, 1]
        if fuse and dtype == f32:
            d2 = (dx.astype(f64) * dx.astype(f64) + (dy * dy).astype(f64)).astype(f32)  # (48 + 24 bits: the sum is exact in double)
        else:
            d2 = dx * dx + dy * dy
        hit[:, j] = d2 <= row[j, 2]
        pen = (pen + np.where(hit[:, j], row[j, 3], dtype(0.0))).astype(dtype)
    return pen, hit


def rollout(P, grid, table, x0, U, dtype=f32, states=None, fuse=False):
    """U [N, T, 2] (already clamped by the solver), table [rows >= T, n, 4] -> dict(costs [N], S [N, T+1, 3], hit [N, T+1, n]
    (index T: the terminal cost, row T-1), near [N], edge [N], scale).  Stage costs are added in double and rounded once
    (CostSum<true>)."""
    U = np.asarray(U)
    N, T, _ = U.shape
    table = np.asarray(table, f32)
    n = table.shape[1]
    assert table.shape[0] >= T and n <= MAX_DISCS
    Ud = U.astype(dtype)
    s = np.broadcast_to(np.asarray(x0, f32).astype(dtype), (N, 3)).copy()
    S = np.empty((N, T + 1, 3), dtype)
    H = np.zeros((N, T + 1, n), bool)
    acc = np.zeros(N, f64)
    near, edge = np.zeros(N, bool), np.zeros(N, bool)
    for t in range(T + 1):
        if states is not None:
            s = np.asarray(states[:, t], f32).astype(dtype)
        S[:, t] = s
        row = table[min(t, T - 1)]
        pen, H[:, t] = penalty(row, n, s[:, 0], s[:, 1], dtype, fuse)
        c = (base_cost(P, grid, s, dtype) + pen).astype(dtype)
        acc += c.astype(f64)
        if dtype == f64:
            for j in range(n):
                d = np.sqrt((s[:, 0] - f64(row[j, 0])) ** 2 + (s[:, 1] - f64(row[j, 1])) ** 2)
                if row[j, 2] >= 0:
                    near |= np.abs(d - np.sqrt(f64(row[j, 2]))) <= NEAR_M
            e = EDGE_CELLS * grid[1]
            o = occupancy(grid, s[:, 0], s[:, 1], f64)
            for ex, ey in ((e, e), (e, -e), (-e, e), (-e, -e)):
                edge |= occupancy(grid, s[:, 0] + ex, s[:, 1] + ey, f64) != o
        if t < T and states is None:
            s = step(P, s, Ud[:, t], dtype)
    costs = acc.astype(f32) if dtype == f32 else acc
    return dict(costs=costs, S=S, hit=H, near=near, edge=edge, scale=float(np.max(np.abs(acc))))


def padded(table):
    """[rows, n, 4] -> the device's [rows, 8, 4]"""
    table = np.asarray(table, f32)
    out = np.broadcast_to(PAD, (table.shape[0], MAX_DISCS, 4)).copy()
    out[:, :table.shape[1]] = table
    return out


def actions(seed, N, T, mean=MEAN):
    """Clamped random actions like the solver's around `mean`"""
    rng = np.random.default_rng(seed)
    return np.clip(mean + rng.standard_normal((N, T, 2)) * SIGMAS, U_MIN, U_MAX).astype(f32)


# ---------------------------------------------------------------------------------------------- the case table
# Placed by hand along the path of the mean action (v = 1 m/s along the start heading pi/4, 0.1 m per step):
# p(t) = start + 0.1 t h.  `ahead` is measured along h, `side` along the left normal, velocities in m/s (<= 1).
_H = np.array([np.cos(np.pi / 4), np.sin(np.pi / 4)])
_L = np.array([-_H[1], _H[0]])
FAR = f32([50.0, 50.0, 0.04, 3.0])  # a real disc nobody reaches (the map ends at 10 m)


def _moving(start, T, specs):
    """specs: (t_cross, ahead offset, side offset at t_cross, (v_ahead, v_side), radius, weight) -> table [T, n, 4]"""
    tab = np.zeros((T, len(specs), 4), f64)
    for j, (tc, da, dsd, (va, vs), r, w) in enumerate(specs):
        assert np.hypot(va, vs) <= 1.0 + 1e-12 and 0.15 <= r <= 0.45
        for t in range(T):
            c = start[:2].astype(f64) + (0.1 * tc + da + va * 0.1 * (t - tc)) * _H + (dsd + vs * 0.1 * (t - tc)) * _L
            tab[t, j] = [c[0], c[1], r * r, w]
    return tab.astype(f32)


def _only_row(T, t_row, disc, n=1, slot=0):
    tab = np.broadcast_to(FAR, (T, n, 4)).copy()
    tab[t_row, slot] = disc
    return tab


def _crossing(T, n, start=X0):
    """n discs that cross the path in the later part of the horizon, from alternating sides.  The samples are spread along
    the path (about 0.05 sqrt(t) m at step t) and hardly across it, so each disc crosses BEHIND the mean position by its
    radius plus part of that spread and falls back further: only the slower samples meet it.  (Sideways at 0.097 m per
    step: no radius of the table is a multiple of it, so no disc is TANGENT to the line the samples lie on early on.)"""
    specs = []
    for j in range(n):
        tc = min(T, max(1, round(T * (0.45 + 0.5 * (j + 1) / (n + 1)))))
        side = 1.0 if j % 2 == 0 else -1.0
        r = 0.2 if n == 1 else 0.15 + (0.05 if n <= 3 else 0.02) * (j % 4)
        gap = r + (0.2 if n == 1 else 1.6 if n <= 3 else 2.1) * 0.05 * np.sqrt(tc) + (0.01 * j if tc <= 2 else 0.0)
        specs.append((tc, -gap, 0.0, (-0.2, 0.97 * side), r, 10.0 * (j + 1)))
    return _moving(start, T, specs)


def _step0(T):     # the stage cost of step 0 sees the start pose itself: every sample is hit there (the terminal cost of T = 1
    return _only_row(T, 0, [X0[0] - 0.07, X0[1] - 0.07, 0.15 ** 2, 7.0])  # reads row 0 as well)


def _stage_last(T):  # row T-1 only, its FRONT edge 0.05 m beyond where the mean path is at step T-1: the samples just short of
    c = X0[:2] + (0.1 * (T - 1) + 0.05 - 0.3) * _H                        # the edge leave the disc with their last step
    return _only_row(T, T - 1, [c[0], c[1], 0.3 ** 2, 5.0])


def _terminal(T):    # row T-1 too, its BACK edge 0.05 m short of where the mean path ENDS: the samples just short of that edge
    c = X0[:2] + (0.1 * T - 0.05 + 0.3) * _H                              # enter with their last step, seen by the terminal cost only
    return _only_row(T, T - 1, [c[0], c[1], 0.3 ** 2, 5.0])


def _slot7(T):
    tab = np.broadcast_to(FAR, (T, 8, 4)).copy()
    tab[:, 7] = _crossing(T, 1)[:, 0]
    return tab


def _overlap8(T):
    return np.repeat(_crossing(T, 1), 8, axis=1) * f32([1, 1, 1, 0.25])  # eight copies, w = 2.5 each: pen = 8 w


# eight distinct weights whose fp32 sum depends on the order: behind 8192 (ulp 0.00098) each small one is rounded away,
# ahead of it they add up to two ulps
WEIGHTS8 = f32([8192.0, 0.00030, 0.00031, 0.00032, 0.00033, 0.00034, 0.00035, 0.00036])


def _weights8(T):
    tab = np.repeat(_crossing(T, 1), 8, axis=1)
    tab[:, :, 3] = WEIGHTS8
    return tab


# name -> (table(T), start pose)
CASES = {
    "step0": (_step0, X0), "stage_last": (_stage_last, X0), "terminal": (_terminal, X0), "slot7": (_slot7, X0),
    "overlap8": (_overlap8, X0), "weights8": (_weights8, X0),
    "n0": (lambda T: np.zeros((T, 0, 4), f32), X0), "n1": (lambda T: _crossing(T, 1), X0),
    "n3": (lambda T: _crossing(T, 3), X0), "n8": (lambda T: _crossing(T, 8), X0),
    "x0out": (lambda T: _crossing(T, 3, X0_OUT), X0_OUT),
}
MIXED = ("n1", "n3", "n8", "slot7", "overlap8", "weights8")  # hit share between 5 % and 95 % (at the horizons >= 7)


def case(name, T):
    fn, x0 = CASES[name]
    return np.ascontiguousarray(fn(T), f32), x0
