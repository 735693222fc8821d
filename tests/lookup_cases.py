"""Geometries and points for the map lookup inside the nav2d and racing cost kernels (occ_lookup / occ_lookup_pad in
csrc/mppi_models.inc, pad_map_plan in csrc/mppi_models.hpp, refresh_pad / pad_map_kernel on the device).

The vehicle is held still (nav2d: zero mean and zero injected noise make the speed 0; racing: start speed 0 and zero
acceleration), so stage 0 of every sample looks up the start x0 as given and every later stage, the terminal one included,
looks up clamp(x0): the total cost of a horizon of T steps holds occ(x0) + T * occ(clamp(x0)) as an integer that decodes with
no tolerance (decode_nav2d / decode_racing).  The reference is the oracle's lookup: fp32 x / cell + origin, rintf, out of
grid = 1.

numpy only: nothing here touches the GPU or the library.  tests/test_lookup_cases_host.py asserts that the set reaches what
it claims (ties, the pad ring, clamped starts, wrong lookups told apart) and sweeps the host build of the header;
tests/test_gpu_map_lookup.py runs the set on the device.
"""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass

import numpy as np

f32 = np.float32
T = 3              # horizon of the stationary rollouts: occ(x0) + T * occ(clamp(x0)) decodes uniquely for values 0..2
N = 64             # samples per rollout (all must agree to the bit)
QO_NAV2D = 1024.0  # nav2d's obstacle weight: a power of two far above any goal distance's rounding error
CAP = 256          # points per geometry on the device
MAGIC = f32(12582912.0)  # 1.5 * 2^23

CELL_BELOW = float(np.nextafter(f32(0.125), f32(0)))  # all-ones significand: no Markstein reciprocal, level 0
CELL_ABOVE = float(np.nextafter(f32(0.125), f32(1)))  # its neighbour on the other side stays fast
CELLS = (0.1, 0.05, 0.125, 0.3, 1.0)
ORIGINS = ("half", "zero", "last", "frac")
LIMITS = ("exact", "inside", "beyond")
TINY = ((1, 1), (1, 7), (7, 1), (5, 7), (64, 3), (3, 64))
LONG = (255, 256, 1022, 1023, 1024, 4095)


# ------------------------------------------------------------------------------ float32 helpers
def _key(x):
    """float32 -> int64 that orders like the floats (-0.0 just below +0.0)"""
    b = np.asarray(x, f32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF) - 1, b)


def _unkey(k):
    k = np.asarray(k, np.int64)
    b = np.where(k < 0, (-(k + 1)) | 0x80000000, k).astype(np.uint32)
    return b.view(f32)


def ulp_step(x, n):
    """the float32 n steps above (n < 0: below) x"""
    return _unkey(_key(x) + n)


def coord(x, cell, o):
    """the reference's cell coordinate: fp32 x / cell + origin (two roundings)"""
    with np.errstate(over="ignore"):
        return (np.asarray(x, f32) / f32(cell) + f32(o)).astype(f32)


def all_ones(cell):
    return (int(f32(cell).view(np.uint32)) & 0x7FFFFF) == 0x7FFFFF


def _extreme(cell, o, pred, want_smallest, guess):
    """smallest / largest float32 x within a few cells of `guess` whose coordinate satisfies the monotone predicate"""
    lo, hi = int(_key(f32(guess - 3 * cell))), int(_key(f32(guess + 3 * cell)))
    ok = lambda k: bool(pred(coord(_unkey(k), cell, o)))  # noqa: E731
    if want_smallest:  # pred is False ... True along x
        assert not ok(lo) and ok(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if ok(mid) else (mid, hi)
        return float(_unkey(hi))
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return float(_unkey(lo))


def hit(q, cell, o):
    """a float32 x whose coordinate is exactly the float32 q (the nearest of the few floats around (q - o) * cell), or None"""
    q = f32(q)
    est = f32((float(q) - float(f32(o))) * float(f32(cell)))
    cand = ulp_step(est, np.array([0, 1, -1, 2, -2, 3, -3]))
    ok = coord(cand, cell, o) == q
    return float(cand[np.argmax(ok)]) if ok.any() else None


def near(q, cell, o):
    return hit(q, cell, o) if hit(q, cell, o) is not None else float(f32((float(q) - float(f32(o))) * float(f32(cell))))


# ------------------------------------------------------------------------------ geometries
@dataclass(frozen=True)
class Geometry:
    name: str
    family: str
    nx: int
    ny: int
    cell: float
    origin: tuple    # (ox, oy), float32 values
    x_lim: tuple     # float32 values
    y_lim: tuple
    limits: str      # "exact" | "inside" | "beyond"
    seed: int

    @property
    def tiny(self):
        return self.family == "tiny" or (self.nx + 1) * (self.ny + 1) <= 64

    def grids(self):
        """(obstacle grid, lane grid, another lane grid of the same geometry): seeded random 0/1"""
        rng = np.random.default_rng(self.seed)
        return tuple((rng.random((self.nx, self.ny)) < p).astype(np.uint8) for p in (0.4, 0.5, 0.5))

    def box_in_pad(self):
        """every index the position clamp can reach lies in [0, nx] x [0, ny] (the coordinate is monotone: the box's four
        limits decide) — what the padded lookup needs.  tests/test_lookup_cases_host.py holds this to a brute-force check."""
        out = True
        for (lo, hi), o, n in ((self.x_lim, self.origin[0], self.nx), (self.y_lim, self.origin[1], self.ny)):
            out = out and bool(np.rint(coord(lo, self.cell, o)) >= 0 and np.rint(coord(hi, self.cell, o)) <= n)
        return out

    def fast(self):
        """the level-1/2 kernels apply: a usable reciprocal of the cell size, and the padded grid serves the whole box"""
        return not all_ones(self.cell) and self.box_in_pad() and self.nx < (1 << 20) and self.ny < (1 << 20)

    def level(self, math):
        return int(math) if self.fast() else 0

    def goal(self):
        """nav2d's goal: the middle of the box"""
        return (float(f32(0.5 * (self.x_lim[0] + self.x_lim[1]))), float(f32(0.5 * (self.y_lim[0] + self.y_lim[1]))))


def _origin(kind, n):
    return float(f32({"half": n // 2, "zero": 0, "last": n - 1, "frac": n / 2 + 0.25}[kind]))


def _limits(kind, n, cell, o):
    if kind == "exact":  # the largest box whose rounded indices stay in [0, n]: its upper limit indexes the pad ring
        return (_extreme(cell, o, lambda q: np.rint(q) >= 0, True, (-0.5 - o) * cell),
                _extreme(cell, o, lambda q: np.rint(q) <= n, False, (n + 0.5 - o) * cell))
    if kind == "inside":  # strictly inside the grid
        qlo, qhi = (1.0, n - 2.0) if n >= 4 else (-0.25, n - 0.75)
        return near(qlo, cell, o), near(qhi, cell, o)
    return near(-1.0, cell, o), near(n + 1.0, cell, o)  # one cell beyond on either side: the plan must refuse it


def make(name, family, nx, ny, cell, okind, limits, seed):
    cell = float(f32(cell))
    ox, oy = _origin(okind, nx), _origin(okind, ny)
    return Geometry(name, family, nx, ny, cell, (ox, oy), _limits(limits, nx, cell, ox), _limits(limits, ny, cell, oy), limits, seed)


@functools.lru_cache(maxsize=None)
def geometries():
    out, seed = [], 0
    shapes = [("tiny", s) for s in TINY] + [("long_y", (3, n)) for n in LONG] + [("long_x", (n, 3)) for n in LONG]
    for i, (fam, (nx, ny)) in enumerate(shapes):  # every shape with the three kinds of limits; cell and origin rotate
        for j, lim in enumerate(LIMITS):
            cell, okind = CELLS[(i + j) % len(CELLS)], ORIGINS[(i + 2 * j + 1) % len(ORIGINS)]
            seed += 1
            out.append(make(f"{fam}-{nx}x{ny}-c{cell:g}-{okind}-{lim}", fam, nx, ny, cell, okind, lim, seed))
    for nx, ny in ((5, 7), (3, 1023), (1024, 3)):  # every cell size, the all-ones one and its neighbour included
        for cell, tag in [(c, f"{c:g}") for c in CELLS] + [(CELL_BELOW, "0.125-"), (CELL_ABOVE, "0.125+")]:
            for lim in ("exact", "inside") if tag[-1] in "-+" else ("exact",):
                seed += 1
                out.append(make(f"cell-{nx}x{ny}-c{tag}-half-{lim}", "cell", nx, ny, cell, "half", lim, seed))
    for nx, ny in ((5, 7), (3, 1023), (4095, 3)):  # every origin
        for okind in ORIGINS:
            seed += 1
            out.append(make(f"origin-{nx}x{ny}-c0.1-{okind}-exact", "origin", nx, ny, 0.1, okind, "exact", seed))
    for nx, ny in ((5, 7), (3, 1023), (1024, 3)):  # the largest box with ONE limit moved one float outward: index -1 or n + 1
        for side in ("xlo", "xhi", "ylo", "yhi"):
            seed += 1
            g = make(f"edge-{nx}x{ny}-c0.1-half-exact+{side}", "edge", nx, ny, 0.1, "half", "exact", seed)
            lim = {"x": list(g.x_lim), "y": list(g.y_lim)}
            lim[side[0]][side[1:] == "hi"] = float(ulp_step(f32(lim[side[0]][side[1:] == "hi"]), 1 if side[1:] == "hi" else -1))
            out.append(dataclasses.replace(g, x_lim=tuple(lim["x"]), y_lim=tuple(lim["y"]), limits="beyond"))
    assert len({g.name for g in out}) == len(out)
    return tuple(out)


def families():
    return tuple(sorted({g.family for g in geometries()}))


def by_family(family):
    return tuple(g for g in geometries() if g.family == family)


def by_name(name):
    return next(g for g in geometries() if g.name == name)


# ------------------------------------------------------------------------------ points
def axis_points(n, cell, o, lim):
    """positions along one axis: for the indices {0, 1, mid, n-2, n-1, n} the cell centre, both ties, each tie moved one ulp
    of the coordinate and one ulp of the position either way; both clamp limits with their neighbours; far out; +-0"""
    xs = []
    for i in sorted({0, 1, n // 2, n - 2, n - 1, n} & set(range(0, n + 1))):
        xs.append(hit(f32(i), cell, o))
        for tie in (f32(i - 0.5), f32(i + 0.5)):
            for q in (tie, np.nextafter(tie, f32(-np.inf)), np.nextafter(tie, f32(np.inf))):
                xs.append(hit(q, cell, o))
            x = hit(tie, cell, o)
            if x is not None:
                xs += [float(ulp_step(f32(x), -1)), float(ulp_step(f32(x), 1))]
    for v in lim:
        xs += [v, float(ulp_step(f32(v), -1)), float(ulp_step(f32(v), 1))]
    xs += [near(-1000.0, cell, o), near(n + 1000.0, cell, o), 0.0, -0.0]
    seen, out = set(), []
    for x in xs:
        if x is None:
            continue
        k = int(_key(f32(x)))
        if k not in seen:
            seen.add(k)
            out.append(f32(x))
    return np.array(out, f32)


@functools.lru_cache(maxsize=None)
def points(g, cap=None):
    """[n][2] float32 start positions of geometry g.  cap = None: the full cross of both axes' lists (host sweeps); with a cap,
    a fixed subset for the device: every per-axis value paired twice, the tiny grids' cells and pad ring, and a seeded fill."""
    xs, ys = axis_points(g.nx, g.cell, g.origin[0], g.x_lim), axis_points(g.ny, g.cell, g.origin[1], g.y_lim)
    ring = []
    if g.tiny:  # every cell and every pad-ring cell once at its centre: nothing else observes the pad grid's copy
        for ix in range(g.nx + 1):
            for iy in range(g.ny + 1):
                ring.append((near(f32(ix), g.cell, g.origin[0]), near(f32(iy), g.cell, g.origin[1])))  # (within an ulp of it)
    ring = np.array(ring, f32).reshape(-1, 2)
    if cap is None:
        cross = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
        return np.concatenate([ring, cross]).astype(f32)
    a, b = len(xs), len(ys)
    k = np.arange(max(a, b))
    pairs = np.concatenate([np.stack([xs[k % a], ys[k % b]], 1), np.stack([xs[k % a], ys[(5 * k + 3) % b]], 1),
                            np.stack([xs[(7 * k + 2) % a], ys[k % b]], 1)])
    rng = np.random.default_rng(g.seed)
    fill = np.stack([xs[rng.integers(0, a, cap)], ys[rng.integers(0, b, cap)]], 1)
    return np.concatenate([ring, pairs, fill])[:max(cap, len(ring) + len(pairs))].astype(f32)


# ------------------------------------------------------------------------------ the lookup in numpy, and wrong ones
def lookup(g, grid, pts, *, rounding="even", quotient="divide", swap=False, oob=1, index_bits=None):
    """The reference lookup (defaults) on an [nx][ny] grid, restated so that single decisions can be got wrong."""
    pts = np.asarray(pts, f32).reshape(-1, 2)
    px, py = (pts[:, 1], pts[:, 0]) if swap else (pts[:, 0], pts[:, 1])
    if quotient == "divide":
        qx, qy = coord(px, g.cell, g.origin[0]), coord(py, g.cell, g.origin[1])
    else:  # one multiply by RN(1 / cell)
        inv = f32(1.0) / f32(g.cell)
        with np.errstate(over="ignore"):
            qx, qy = (px * inv + f32(g.origin[0])).astype(f32), (py * inv + f32(g.origin[1])).astype(f32)
    q = np.stack([qx, qy], 1).astype(np.float64)
    if rounding == "even":
        i = np.rint(q)
    elif rounding == "away":
        i = np.sign(q) * np.floor(np.abs(q) + 0.5)
    else:  # floor(q + 0.5) in float32
        i = np.floor((q.astype(f32) + f32(0.5)).astype(f32)).astype(np.float64)
    i = np.clip(i, -2.0 ** 40, 2.0 ** 40).astype(np.int64)
    ix, iy = i[:, 0], i[:, 1]
    inb = (ix >= 0) & (ix < g.nx) & (iy >= 0) & (iy < g.ny)
    if index_bits is not None:
        ix = ix & ((1 << index_bits) - 1)
    lin = np.where(inb, ix * g.ny + iy, 0)
    lin = np.clip(lin, 0, grid.size - 1)
    return np.where(inb, grid.reshape(-1)[lin], oob).astype(np.int64)


def lookup_pad(g, grid, pts, *, stride=None, ring=1):
    """The lookup on the (nx+1) x (ny+1) padded copy, for points whose indices lie in [0, nx] x [0, ny]; a wrong row stride
    reads the copy as the device would (flat, clipped to the buffer)."""
    pts = np.asarray(pts, f32).reshape(-1, 2)
    pad = np.full((g.nx + 1, g.ny + 1), ring, np.int64)
    pad[:g.nx, :g.ny] = grid
    ix = np.rint(coord(pts[:, 0], g.cell, g.origin[0])).astype(np.int64)
    iy = np.rint(coord(pts[:, 1], g.cell, g.origin[1])).astype(np.int64)
    lin = ix * (g.ny + 1 if stride is None else stride) + iy
    return pad.reshape(-1)[np.clip(lin, 0, pad.size - 1)]


def clamp(g, pts):
    pts = np.asarray(pts, f32).reshape(-1, 2)
    return np.stack([np.clip(pts[:, 0], f32(g.x_lim[0]), f32(g.x_lim[1])), np.clip(pts[:, 1], f32(g.y_lim[0]), f32(g.y_lim[1]))], 1)


def in_box(g, pts):
    pts = np.asarray(pts, f32).reshape(-1, 2)
    return ((pts[:, 0] >= f32(g.x_lim[0])) & (pts[:, 0] <= f32(g.x_lim[1])) & (pts[:, 1] >= f32(g.y_lim[0])) & (pts[:, 1] <= f32(g.y_lim[1])))


def margins(g, pts):
    """[n][2]: distance of each coordinate from its rounding tie, as the oracle measures it (exactly 0 on a tie)"""
    pts = np.asarray(pts, f32).reshape(-1, 2)
    q = np.stack([coord(pts[:, 0], g.cell, g.origin[0]), coord(pts[:, 1], g.cell, g.origin[1])], 1)
    return np.abs((q - np.floor(q)).astype(f32) - f32(0.5))


def indices(g, pts):
    pts = np.asarray(pts, f32).reshape(-1, 2)
    return np.stack([np.rint(coord(pts[:, 0], g.cell, g.origin[0])), np.rint(coord(pts[:, 1], g.cell, g.origin[1]))], 1)


def counts(g, pts, model, fn=None):
    """the decoded integer a stationary rollout of T steps must give: value(x0) + T * value(clamp(x0)); racing sums both grids.
    `fn(grid, pts, stage)` replaces the lookup (the wrong ones of the host test)."""
    grids = g.grids()[:2 if model == "racing" else 1]
    fn = fn or (lambda grid, p, stage: lookup(g, grid, p))
    return sum(fn(grid, pts, 0) + T * fn(grid, clamp(g, pts), 1) for grid in grids)


# ------------------------------------------------------------------------------ the rollout's inputs and the decoding
def nav2d_params(g):
    gx, gy = g.goal()
    return [0.0, 2.0, -1.0, 1.0, 0.1, g.x_lim[0], g.x_lim[1], g.y_lim[0], g.y_lim[1], gx, gy, QO_NAV2D]


def racing_params(g, u_min=(-2.0, -0.25), u_max=(2.0, 0.25), L=1.0):
    return [u_min[0], u_max[0], u_min[1], u_max[1], L, 8.0, 0.1, g.x_lim[0], g.x_lim[1], g.y_lim[0], g.y_lim[1],
            0.0, 0.0, 0.0, 1.0, 0.0, 0.0]  # Qc = Ql = Qv = 0, Qo = 1, Qin = Qdin = 0


U_BOUNDS = {"nav2d": ((0.0, -1.0), (2.0, 1.0)), "racing": ((-2.0, -0.25), (2.0, 0.25))}
DIMS = {"nav2d": (3, 2), "racing": (4, 2)}


def params(g, model):
    return nav2d_params(g) if model == "nav2d" else racing_params(g)


def maps(g, model):
    a, b, _ = g.grids()
    return [(a, g.cell, g.origin)] + ([(b, g.cell, g.origin)] if model == "racing" else [])


def states(g, pts, model):
    """start states [n][ds]: the position, heading 0 (racing: speed 0)"""
    pts = np.asarray(pts, f32).reshape(-1, 2)
    s = np.zeros((len(pts), DIMS[model][0]), f32)
    s[:, :2] = pts
    return s


def reference_rows(g):
    """racing's constant reference: T + 1 rows of {x, y, yaw, v} at the goal, yaw 0, speed 0"""
    gx, gy = g.goal()
    return np.tile(np.array([gx, gy, 0.0, 0.0], f32), (T + 1, 1))


def decode(g, pts, costs, model):
    """(k, guard): the integer count held by each total cost, and the distance of the cost from what k stands for.
    racing: the cost IS the count.  nav2d: cost - (g0 + T * g1) with the goal distances of x0 and clamp(x0) in float64."""
    costs = np.asarray(costs, np.float64)
    if model == "racing":
        k = np.rint(costs)
        return k.astype(np.int64), np.abs(costs - k)
    pts = np.asarray(pts, f32).reshape(-1, 2)
    goal = np.array(g.goal(), f32).astype(np.float64)
    dist = lambda p: np.sqrt(((p.astype(np.float64) - goal) ** 2).sum(1))  # noqa: E731
    rest = costs - (dist(pts) + T * dist(clamp(g, pts)))
    k = np.rint(rest / QO_NAV2D)
    return k.astype(np.int64), np.abs(rest - k * QO_NAV2D)
