"""numpy restatement of racing among moving discs (MPPI_MODEL_RACING_DISCS: csrc/mppi_models.inc, csrc/mppi_discs.hpp;
include/mppi_hip.h, mppi_set_discs, states the rule) and the case table the CPU and the GPU tests share.

  step / cost / rollout in fp32 — every operation rounded on its own, in the functor's order, sinf / cosf / tanf from the C
  library the host build of the functor links (so the two agree bit for bit), fmod exact in any library — and in float64 (the
  yardstick of the fast levels).  The stage costs are summed sequentially in fp32 (CostSum<false>, racing's), the penalty of
  the row's discs is added LAST: cost = (path + velocity + obstacle + input) + pen.
  The stage cost of step t reads reference row t and disc row t, the terminal cost row T-1 of both (there is no row T).
  rollout(..., states=S) evaluates the costs on GIVEN states (a device's own: its sin / cos / tan are another library's, every
  operation of the cost — subtract, multiply, add, divide, round, compare — is exactly rounded everywhere).

Boundary rule of the fast levels (discs_ref.py's): a sample is left out of a cost comparison when, in float64, some (t, j)
has |dist - r| <= 1e-4 m (`near`), or a map-cell rounding lies within 1e-3 cell of a cell of another value (`edge`).
cap(N) = max(2, 0.02 N) bounds how many `near` samples a case may leave out: a condition on the table, not a measurement.
"""
import ctypes
import ctypes.util

import numpy as np

from discs_ref import MAX_DISCS, NEAR_M, EDGE_CELLS, PAD, PARITY, cap, penalty  # noqa: F401  (one owner of the disc rule)

f32, f64 = np.float32, np.float64
REF_ROW, DISC_ROW = 8, 32
KROW = REF_ROW + DISC_ROW  # floats per step of the handle's table: the reference row, then the eight padded discs
PI_F, TWO_PI_F = f32(3.14159274), f32(6.28318548)
V0 = f32(4.0)                    # the speed the cases start at (the example starts at rest: no sample moves in 8 steps)
MEAN, SIGMAS, U_MIN, U_MAX = f32([0.0, 0.0]), f32([0.5, 0.1]), f32([-2.0, -0.25]), f32([2.0, 0.25])
SAMPLES = (64, 100, 4160)        # one tile, a ragged tile, more than the single launch takes
HORIZONS = (1, 2, 3, 7, 8, 25)   # dc = 2, two steps per float4 group: the group loop, both drain halves, a ragged and a complete epilogue
COUNTS = (0, 1, 3, 8)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf", "tanf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]
_sinf = np.frompyfunc(lambda v: _libm.sinf(float(v)), 1, 1)
_cosf = np.frompyfunc(lambda v: _libm.cosf(float(v)), 1, 1)
_tanf = np.frompyfunc(lambda v: _libm.tanf(float(v)), 1, 1)


def _sin(x, dtype):
    return _sinf(x).astype(f32) if dtype == f32 else np.sin(x)


def _cos(x, dtype):
    return _cosf(x).astype(f32) if dtype == f32 else np.cos(x)


def _tan(x, dtype):
    return _tanf(x).astype(f32) if dtype == f32 else np.tan(x)


def angle_normalize(x, dtype):
    """((x + pi) % 2 pi) - pi with torch.remainder semantics (fmod + sign fix); fmod is exact in any library"""
    pi, two_pi = dtype(PI_F), dtype(TWO_PI_F)
    r = np.fmod(x + pi, two_pi)
    r = np.where((r != 0) & (r < 0), r + two_pi, r)
    return (r - pi).astype(dtype)


def step(P, s, u, dtype=f32):
    """Model<RACING>::step at math level 0: P = the 17 MPPI_RP_* parameters, s [N, 4], u [N, 2] -> next state [N, 4]"""
    P = np.asarray(P, f32).astype(dtype)
    accel = np.clip(u[:, 0], P[0], P[1])
    steer = np.clip(u[:, 1], P[2], P[3])
    x, y, v = s[:, 0], s[:, 1], s[:, 3]
    th = angle_normalize(s[:, 2], dtype)
    sn, cs = _sin(th, dtype), _cos(th, dtype)
    dx, dy = v * cs, v * sn
    vt = v * _tan(steer, dtype)
    dth = vt / P[4]
    nx = x + dx * P[6]
    ny = y + dy * P[6]
    nth = angle_normalize(th + dth * P[6], dtype)
    nv = v + accel * P[6]
    return np.stack([np.clip(nx, P[7], P[8]), np.clip(ny, P[9], P[10]), nth, np.clip(nv, -P[5], P[5])], 1).astype(dtype)


def occupancy(grid, x, y, dtype=f32):
    """occ_lookup: idx = round_half_even(p / cell + origin); out of bounds -> 1"""
    cells, cell, ox, oy = grid
    qx = np.rint(x / dtype(f32(cell)) + dtype(f32(ox)))
    qy = np.rint(y / dtype(f32(cell)) + dtype(f32(oy)))
    ix, iy = qx.astype(np.int64), qy.astype(np.int64)
    inb = (ix >= 0) & (ix < cells.shape[0]) & (iy >= 0) & (iy < cells.shape[1])
    v = cells[np.clip(ix, 0, cells.shape[0] - 1), np.clip(iy, 0, cells.shape[1] - 1)].astype(dtype)
    return np.where(inb, v, dtype(1.0))


def occupancy2(grids, x, y, dtype=f32):
    return (occupancy(grids[0], x, y, dtype) + occupancy(grids[1], x, y, dtype)).astype(dtype)


def ref_rows(ref, dtype=f32):
    """[rows, 4] = (x, y, yaw, v) -> [rows, 8] as mppi_set_reference stages it: sin / cos of the fp32 yaw by the C library
    (float64: of the same fp32 yaw, in double)"""
    ref = np.asarray(ref, f32)
    out = np.zeros((ref.shape[0], REF_ROW), dtype)
    out[:, :4] = ref.astype(dtype)
    out[:, 4], out[:, 5] = _sin(ref[:, 2] if dtype == f32 else ref[:, 2].astype(f64), dtype), _cos(ref[:, 2] if dtype == f32 else ref[:, 2].astype(f64), dtype)
    return out


def base_cost(P, grids, k, s, u, pu, dtype=f32):
    """Model<RACING>::cost: k = one row of ref_rows; s [N, 4]; u, pu [N, 2]"""
    P = np.asarray(P, f32).astype(dtype)
    xr, yr, vr, sinp, cosp = k[0], k[1], k[3], k[4], k[5]
    ex, ey = s[:, 0] - xr, s[:, 1] - yr
    ec = sinp * ex - cosp * ey
    el = (-cosp) * ex - sinp * ey
    path = P[11] * (ec * ec) + P[12] * (el * el)
    dv = s[:, 3] - vr
    vel = P[13] * (dv * dv)
    obst = P[14] * occupancy2(grids, s[:, 0], s[:, 1], dtype)
    inp = P[15] * (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1])
    d0, d1 = u[:, 0] - pu[:, 0], u[:, 1] - pu[:, 1]
    inp = inp + P[16] * (d0 * d0 + d1 * d1)
    return (((path + vel) + obst) + inp).astype(dtype)


def rollout(P, grids, ref, table, x0, U, dtype=f32, states=None, fuse=False):
    """U [N, T, 2] (already clamped by the solver), ref [rows >= T, 4], table [rows >= T, n, 4] -> dict(costs [N],
    S [N, T+1, 4], hit [N, T+1, n] (index T: the terminal cost, row T-1), near [N], edge [N], scale).  The recorded state of
    step t is the state the step starts from (step 0: the start itself, heading unwrapped)."""
    U = np.asarray(U)
    N, T, _ = U.shape
    table = np.asarray(table, f32)
    n = table.shape[1]
    K = ref_rows(ref, dtype)
    assert table.shape[0] >= T and K.shape[0] >= T and n <= MAX_DISCS
    Ud = U.astype(dtype)
    s = np.broadcast_to(np.asarray(x0, f32).astype(dtype), (N, 4)).copy()
    S = np.empty((N, T + 1, 4), dtype)
    H = np.zeros((N, T + 1, n), bool)
    acc = np.zeros(N, dtype)
    near, edge = np.zeros(N, bool), np.zeros(N, bool)
    zero = np.zeros((N, 2), dtype)
    for t in range(T + 1):
        if states is not None:
            s = np.asarray(states[:, t], f32).astype(dtype)
        S[:, t] = s
        row = min(t, T - 1)
        # info["prev_action"]: step 0 sees U[:, 0] itself, step t U[:, t-1]; the terminal cost a zero action and the stale
        # U[:, max(T-2, 0)] (mppi.py:299-301,318-328)
        u = Ud[:, t] if t < T else zero
        pu = Ud[:, max(t - 1, 0)] if t < T else Ud[:, max(T - 2, 0)]
        pen, H[:, t] = penalty(table[row], n, s[:, 0], s[:, 1], dtype, fuse)
        c = (base_cost(P, grids, K[row], s, u, pu, dtype) + pen).astype(dtype)
        acc = (acc + c).astype(dtype)  # sequential, in the working precision; the terminal cost last
        if dtype == f64:
            for j in range(n):
                d = np.sqrt((s[:, 0] - f64(table[row, j, 0])) ** 2 + (s[:, 1] - f64(table[row, j, 1])) ** 2)
                if table[row, j, 2] >= 0:
                    near |= np.abs(d - np.sqrt(f64(table[row, j, 2]))) <= NEAR_M
            e = EDGE_CELLS * grids[0][1]
            o = occupancy2(grids, s[:, 0], s[:, 1], f64)
            for ex, ey in ((e, e), (e, -e), (-e, e), (-e, -e)):
                edge |= occupancy2(grids, s[:, 0] + ex, s[:, 1] + ey, f64) != o
        if t < T and states is None:
            s = step(P, s, Ud[:, t], dtype)
    return dict(costs=acc, S=S, hit=H, near=near, edge=edge, scale=float(np.max(np.abs(acc.astype(f64)))))


# ---------------------------------------------------------------------------------------------- the table's layout
def padded(table):
    """[rows, n, 4] -> the device's disc part [rows, 8, 4]"""
    table = np.asarray(table, f32)
    out = np.broadcast_to(PAD, (table.shape[0], MAX_DISCS, 4)).copy()
    out[:, :table.shape[1]] = table
    return out


def combined(ref, table):
    """The handle's step table [rows, 40]: floats 0-7 the reference row, floats 8-39 the eight padded discs"""
    ref, table = np.asarray(ref, f32), np.asarray(table, f32)
    rows = min(ref.shape[0], table.shape[0])
    out = np.empty((rows, KROW), f32)
    out[:, :REF_ROW] = ref_rows(ref[:rows])
    out[:, REF_ROW:] = padded(table[:rows]).reshape(rows, DISC_ROW)
    return out


def disc_float(t, j, c=0):
    """index of value c of disc j of step t in the flattened step table"""
    return KROW * t + REF_ROW + 4 * j + c


# ---------------------------------------------------------------------------------------------- the world
def window(center_path, x0, T, v_target=8.0):
    """racing_controller.calc_ref_trajectory from path index 0 (example/racing.py:161-218): [T+1, 4]"""
    p = np.asarray(center_path, f32)
    ind = int(np.argmin(np.hypot(p[:, 0] - f32(x0[0]), p[:, 1] - f32(x0[1]))))
    travel = np.cumsum(np.concatenate([[3.0], np.full(T + 1, 0.85)]))[1:]
    idx = ind + np.rint(travel / 0.1).astype(np.int64)
    assert idx[-1] < len(p)
    out = np.zeros((T + 1, 4), f32)
    out[:, :3] = p[idx]
    out[:, 3] = v_target
    return out


def start_pose(start_state):
    """The example's start pose (position and heading of RacingEnv.reset()) at V0"""
    s = f32(start_state).copy()
    s[3] = V0
    return s


def start_outside(start_state, x_hi):
    """... moved beyond the position clamp (the X0OUT copy of the loop); the first step clamps it back to x_hi"""
    s = start_pose(start_state)
    s[0] = f32(x_hi + 1.5)
    return s


def actions(seed, N, T, mean=MEAN):
    """Clamped random actions like the solver's around `mean`"""
    rng = np.random.default_rng(seed)
    return np.clip(mean + rng.standard_normal((N, T, 2)) * SIGMAS, U_MIN, U_MAX).astype(f32)


# ---------------------------------------------------------------------------------------------- the case table
# Placed along the path of the mean action (no acceleration, no steering): p(t) = start + V0 * 0.1 * t * h along the start
# heading h.  The sampled fan: nothing at steps 0 and 1 (the position of step 1 does not depend on the action), then about
# 0.005 sqrt(t^3 / 3) m along h and 0.016 sqrt(t^3 / 3) m across it.  A disc's edge that cuts the fan where it is narrow
# would put many samples within 1e-4 m of it: every disc below either crosses the path late, where the fan is wide, or keeps
# its edge several fan widths from the path at the early steps.
FAR = f32([500.0, 500.0, 0.04, 3.0])  # a real disc nobody reaches (the track ends at 40 m)
STEP = float(V0) * 0.1
PACE_ROWS = 11


def _frame(x0):
    h = np.array([np.cos(f64(x0[2])), np.sin(f64(x0[2]))])
    return np.asarray(x0[:2], f64), h, np.array([-h[1], h[0]])


def _spread(t):
    return 0.016 * np.sqrt(max(t, 0) ** 3 / 3.0)


def _cars(x0, T, specs):
    """specs: (t_meet, side, radius, speed, weight): a car that drives along h at `speed` < V0 on a line beside the path, its
    edge 0.4 fan widths (a narrow fan: 2) beyond the path — it cuts the fan off-centre — and whose centre the ego's mean
    position draws level with at step t_meet -> table [T, n, 4]"""
    p0, h, left = _frame(x0)
    tab = np.zeros((T, len(specs), 4), f64)
    near = 0.0
    for j, (tm, side, r, speed, w) in enumerate(specs):
        s = _spread(tm)
        lat = side * (r - (0.4 if s >= 0.06 else 2.0) * s + 0.003 * (j + 1))
        # An edge that cuts a fan of width s leaves about 1.6e-4 / s of the samples within 1e-4 m of it, and a car the ego
        # passes slowly stays level for several steps (0.12 % measured at the long horizon).  The smallest sample count of
        # the table is 64 with a cap of 2 samples, so the cars of a table cut the fan while that adds up to 0.37 % — the first
        # one always — and the others drive beside it, a quarter of a metre and three fan widths clear of the path.
        share = max(1.6e-4 / max(s, 1e-3), 0.0012)
        if j and near + share > 0.0037:
            lat = side * (r + 0.25 + 3.0 * s)
        else:
            near += share
        for t in range(T):
            c = p0 + (STEP * tm + speed * 0.1 * (t - tm)) * h + lat * left
            tab[t, j] = [c[0], c[1], r * r, w]
    return tab.astype(f32)


def _crossing(T, n, x0):
    """n slower cars the ego draws level with in the later part of the horizon, on alternating sides"""
    specs = []
    for j in range(n):
        tm = min(T, max(2, round(T * (0.5 + 0.45 * (j + 1) / (n + 1)))))
        specs.append((tm, 1.0 if j % 2 == 0 else -1.0, 0.3 + 0.05 * (j % 4), 1.0 + 0.25 * j, 10.0 * (j + 1)))
    return _cars(x0, T, specs)


def _pace(T, x0):  # one car level with the ego's mean position at EVERY step, the path 0.12 m inside its edge: every sample is
    p0, h, left = _frame(x0)  # hit while the fan is narrower than that, from step 5 on both answers occur at every step; it
    tab = np.zeros((T, 1, 4), f64)  # leaves the track behind row PACE_ROWS - 1 (every step at an edge costs near samples)
    for t in range(T):
        c = p0 + STEP * t * h + (0.4 - 0.12) * left
        tab[t, 0] = [c[0], c[1], 0.4 * 0.4, 20.0] if t < PACE_ROWS else FAR
    return tab.astype(f32)


def _only_row(T, t_row, disc, n=1, slot=0):
    tab = np.broadcast_to(FAR, (T, n, 4)).copy()
    tab[t_row, slot] = disc
    return tab


def _step0(T, x0):   # the stage cost of step 0 sees the start pose itself: every sample is hit there (the terminal cost of
    return _only_row(T, 0, [x0[0] - 0.07, x0[1] - 0.07, 0.15 ** 2, 7.0])  # T = 1 reads row 0 as well, one step further on)


def _terminal(T, x0):  # row T-1 only, its BACK edge 0.05 m short of where the mean path ENDS: the samples enter with their last
    p0, h, _ = _frame(x0)   # step, 0.4 m behind they are outside: only a terminal cost that reads row T-1 sees them
    c = p0 + (STEP * T - 0.05 + 0.3) * h
    return _only_row(T, T - 1, [c[0], c[1], 0.3 ** 2, 5.0])


def _overlap2(T, x0):  # two cars on one spot: the penalties add up
    return np.repeat(_crossing(T, 1, x0), 2, axis=1) * f32([1, 1, 1, 0.25])


def _slot7(T, x0):
    tab = np.broadcast_to(FAR, (T, 8, 4)).copy()
    tab[:, 7] = _crossing(T, 1, x0)[:, 0]
    return tab


# name -> (table(T, x0), start: "in" the position clamp or "out" of it)
CASES = {
    "n0": (lambda T, x0: np.zeros((T, 0, 4), f32), "in"), "n1": (lambda T, x0: _crossing(T, 1, x0), "in"),
    "n3": (lambda T, x0: _crossing(T, 3, x0), "in"), "n8": (lambda T, x0: _crossing(T, 8, x0), "in"),
    "step0": (_step0, "in"), "terminal": (_terminal, "in"), "overlap2": (_overlap2, "in"), "slot7": (_slot7, "in"),
    "pace": (_pace, "in"), "x0out": (lambda T, x0: _crossing(T, 3, x0), "out"),
}
MIXED = ("n1", "n3", "n8", "overlap2", "slot7")  # at the horizons >= 7 some car is hit by 5 % to 95 % of the samples


def case(name, T, start_state, x_hi=40.0):
    """-> (table [T, n, 4], x0 [4])"""
    fn, where = CASES[name]
    x0 = start_pose(start_state) if where == "in" else start_outside(start_state, x_hi)
    # (the x0out case: after the first step the car sits on the clamp's edge; its discs are placed from there)
    place = x0 if where == "in" else f32([x_hi, x0[1], x0[2], x0[3]])
    return np.ascontiguousarray(fn(T, place), f32), x0
