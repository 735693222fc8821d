"""The case set of the in-rollout map lookup (tests/lookup_cases.py) reaches what it claims, tells wrong lookups apart, and
the host build of the header (pad_map_plan, occ_lookup_pad on a pad built as pad_map_kernel builds it, occ_lookup with both
quotients) equals the oracle's lookup on every case point and on a few million random ones per geometry, bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import emul  # noqa: E402
import lookup_cases as lc  # noqa: E402
from oracle import oracle as orc  # noqa: E402

f32 = np.float32
GEOMS = lc.geometries()
IDS = [g.name for g in GEOMS]


def oracle_value(g, model, pts):
    """the oracle's lookup, summed over the model's grids"""
    return sum(orc.occ(grid, g.cell, g.origin, pts) for grid in g.grids()[:2 if model == "racing" else 1]).astype(np.int64)


# ------------------------------------------------------------------------------ the set itself
def test_the_set_covers_every_shape_cell_origin_and_limit_kind():
    shapes = {(g.nx, g.ny) for g in GEOMS}
    assert set(lc.TINY) <= shapes
    assert {(3, n) for n in lc.LONG} | {(n, 3) for n in lc.LONG} <= shapes
    cells = {g.cell for g in GEOMS}
    assert {float(f32(c)) for c in lc.CELLS} | {lc.CELL_BELOW, lc.CELL_ABOVE} <= cells
    assert lc.all_ones(lc.CELL_BELOW) and not lc.all_ones(lc.CELL_ABOVE)
    for fam in ("tiny", "long_x", "long_y"):
        assert {g.limits for g in lc.by_family(fam)} == set(lc.LIMITS)
        assert {g.name.split("-")[3] for g in lc.by_family(fam)} == set(lc.ORIGINS)
    assert any(g.origin[0] != np.rint(g.origin[0]) for g in GEOMS)
    # the levels the set predicts: refused plans and the all-ones cell drop to 0, everything else stays fast
    for g in GEOMS:
        assert g.fast() == (g.limits != "beyond" and g.cell != lc.CELL_BELOW), g.name
    assert any(g.cell == lc.CELL_ABOVE and g.fast() for g in GEOMS)
    # 0x400000 * (ny + 1) exceeds 2^32 from ny = 1023 on: both sides of it are there
    assert {g.ny for g in GEOMS if g.fast()} >= {1022, 1023, 1024, 4095}


@pytest.mark.parametrize("g", GEOMS, ids=IDS)
def test_numpy_lookup_is_the_oracle_lookup(g):
    """lookup_cases.lookup (the base of the wrong lookups below) restates the oracle exactly, on the full cross"""
    pts = lc.points(g)
    for grid in g.grids()[:2]:
        assert np.array_equal(lc.lookup(g, grid, pts), orc.occ(grid, g.cell, g.origin, pts).astype(np.int64))
    inpad = _in_pad(g, pts)
    assert np.array_equal(lc.lookup_pad(g, g.grids()[0], pts[inpad]), lc.lookup(g, g.grids()[0], pts[inpad]))


def _in_pad(g, pts):
    i = lc.indices(g, pts)
    return (i[:, 0] >= 0) & (i[:, 0] <= g.nx) & (i[:, 1] >= 0) & (i[:, 1] <= g.ny)


def _on_ring(g, pts):
    i = lc.indices(g, pts)
    return _in_pad(g, pts) & ((i[:, 0] == g.nx) | (i[:, 1] == g.ny))


@pytest.mark.parametrize("cap", [None, lc.CAP], ids=["full", "capped"])
@pytest.mark.parametrize("family", lc.families())
def test_every_family_reaches_ties_the_pad_ring_and_clamped_starts(family, cap):
    tie_x = tie_y = ring = ring_clamped = moved = False
    seen = set()
    for g in lc.by_family(family):
        pts = lc.points(g, cap)
        assert cap is None or len(pts) <= 2 * cap + 64
        m = lc.margins(g, pts)
        tie_x, tie_y = tie_x or bool((m[:, 0] == 0).any()), tie_y or bool((m[:, 1] == 0).any())
        ring = ring or bool(_on_ring(g, pts).any())
        # a later stage on the ring: reached through the padded lookup itself (in a box the plan accepts)
        ring_clamped = ring_clamped or (g.fast() and bool(_on_ring(g, lc.clamp(g, pts)).any()))
        for model in ("nav2d", "racing"):
            v0, v1 = oracle_value(g, model, pts), oracle_value(g, model, lc.clamp(g, pts))
            moved = moved or bool(((v0 != v1) & ~lc.in_box(g, pts)).any())
            seen |= set(np.unique(v0 + lc.T * v1).tolist())
    assert tie_x and tie_y and ring and moved
    assert ring_clamped or not any(g.fast() for g in lc.by_family(family))  # (the edge family's plans are all refused)
    assert 0 in seen and len(seen) > 2


@pytest.mark.parametrize("g", [g for g in GEOMS if g.family != "cell"], ids=[g.name for g in GEOMS if g.family != "cell"])
def test_every_geometry_has_an_exact_tie_on_each_axis(g):
    m = lc.margins(g, lc.points(g, lc.CAP))
    assert (m[:, 0] == 0).any() and (m[:, 1] == 0).any()


def test_tiny_grids_visit_every_cell_and_every_pad_cell():
    for g in lc.by_family("tiny"):
        for cap in (None, lc.CAP):
            i = lc.indices(g, lc.points(g, cap)).astype(np.int64)
            got = {(a, b) for a, b in i.tolist()}
            assert {(a, b) for a in range(g.nx + 1) for b in range(g.ny + 1)} <= got, g.name


# the wrong lookups: each must differ from the oracle somewhere in the set, or the device test could not fail on it
MUTANTS = {
    "round half away from zero": lambda g, grid, p, st: lc.lookup(g, grid, p, rounding="away"),
    "floor(q + 0.5)": lambda g, grid, p, st: lc.lookup(g, grid, p, rounding="floor"),
    "quotient by one multiply with RN(1/cell)": lambda g, grid, p, st: lc.lookup(g, grid, p, quotient="multiply"),
    "swapped axes": lambda g, grid, p, st: lc.lookup(g, grid, p, swap=True),
    "out-of-grid value 0": lambda g, grid, p, st: lc.lookup(g, grid, p, oob=0),
    "index truncated to 10 bits before the multiply": lambda g, grid, p, st: lc.lookup(g, grid, p, index_bits=10),
    # the padded lookup serves the stages behind the first (and the first of a start inside the box) of a fast geometry
    "padded row stride ny": lambda g, grid, p, st: _padded(g, grid, p, st, stride=g.ny),
    "padded row stride ny + 2": lambda g, grid, p, st: _padded(g, grid, p, st, stride=g.ny + 2),
    "pad ring holding 0": lambda g, grid, p, st: _padded(g, grid, p, st, ring=0),
    "pad ring of the racing sum holding 1": None,  # (see below: needs both grids at once)
    "stage 0 of a start outside the box looked up at the clamped position": None,
}


def _padded(g, grid, p, stage, **kw):
    if not g.fast():
        return lc.lookup(g, grid, p)
    out = lc.lookup(g, grid, p)
    use = lc.in_box(g, p) if stage == 0 else np.ones(len(p), bool)
    out[use] = lc.lookup_pad(g, grid, p[use], **kw)
    return out


@pytest.mark.parametrize("cap", [None, lc.CAP], ids=["full", "capped"])
@pytest.mark.parametrize("model", ["nav2d", "racing"])
@pytest.mark.parametrize("name", list(MUTANTS))
def test_the_case_set_kills_the_mutant(name, model, cap):
    killed_in = []
    for g in GEOMS:
        pts = lc.points(g, cap)
        want = lc.counts(g, pts, model)
        if name.startswith("pad ring of the racing sum"):
            if model != "racing" or not g.fast():
                continue
            a, b, _ = g.grids()
            both = lambda p: lc.lookup_pad(g, a + b, p, ring=1)  # noqa: E731
            v0 = np.where(lc.in_box(g, pts), both(lc.clamp(g, pts)), lc.lookup(g, a, pts) + lc.lookup(g, b, pts))
            got = v0 + lc.T * both(lc.clamp(g, pts))
        elif name.startswith("stage 0"):
            got = (1 + lc.T) * sum(lc.lookup(g, grid, lc.clamp(g, pts)) for grid in g.grids()[:2 if model == "racing" else 1])
        else:
            got = lc.counts(g, pts, model, fn=lambda grid, p, st: MUTANTS[name](g, grid, p, st))
        if not np.array_equal(got, want):
            killed_in.append(g.family)
    if name.startswith("pad ring of the racing sum") and model != "racing":
        return
    assert killed_in, name
    # every mutant but the 10-bit index (which needs a side beyond 1024) dies in the tiny family already
    if "10 bits" in name:
        assert {"long_x", "origin"} <= set(killed_in)
    else:
        assert "tiny" in killed_in, (name, sorted(set(killed_in)))


# ------------------------------------------------------------------------------ the real header on the host
def _brute_force_plan(g, rng):
    """every float of the box's two edges per axis (up to a cap: then the floats next to both ends and a dense sample) and a
    random fill round into [0, nx] x [0, ny]"""
    ok = True
    for (lo, hi), o, n in ((g.x_lim, g.origin[0], g.nx), (g.y_lim, g.origin[1], g.ny)):
        k0, k1 = int(lc._key(f32(lo))), int(lc._key(f32(hi)))
        edge = np.arange(4096)
        ks = np.unique(np.clip(np.concatenate([k0 + edge, k1 - edge, rng.integers(k0, k1 + 1, 1 << 18)]), k0, k1))
        fill = rng.uniform(lo, hi, 1 << 18).astype(f32)
        i = np.rint(lc.coord(np.concatenate([lc._unkey(ks), np.clip(fill, f32(lo), f32(hi))]), g.cell, o))
        ok = ok and bool((i >= 0).all() and (i <= n).all())
    return ok


@pytest.mark.parametrize("g", GEOMS, ids=IDS)
def test_host_build_of_the_header_equals_the_oracle_on_every_case_point(g):
    rng = np.random.default_rng(g.seed)
    pts = lc.points(g)
    for model in ("nav2d", "racing"):
        grids = g.grids()[:2 if model == "racing" else 1]
        r = emul.map_lookup(grids, g.cell, g.origin, g.x_lim, g.y_lim, pts)
        want = oracle_value(g, model, pts)
        # the plan's verdict is the brute-force one, and the case file predicts the gate from it
        assert r["plan"] == _brute_force_plan(g, rng) == g.box_in_pad(), g.name
        assert (r["plan"] and r["usable"]) == g.fast()
        assert r["usable"] == (not lc.all_ones(g.cell))
        if r["plan"]:
            assert r["koff"] + (g.nx + 1) * (g.ny + 1) < 1 << 32
            assert r["koff"] == (0x400000 * (g.ny + 1) + 0x4B400000) % (1 << 32)
        assert np.array_equal(r["lib"].astype(np.int64), want)
        if r["usable"]:
            assert np.array_equal(r["fast"].astype(np.int64), want)
        inside = lc.in_box(g, pts)
        if g.fast():
            assert inside.any() and (r["pad"][~inside] == -1).all()
            assert np.array_equal(r["pad"][inside].astype(np.int64), want[inside])
        else:
            assert (r["pad"] == -1).all()


def test_koff_wraps_in_the_long_geometries():
    """koff = 0x400000 * (ny + 1) + 0x4B400000 is kept mod 2^32: the set holds accepted plans on both sides of the wrap, and on
    both sides of ny = 1023, where the product alone passes 2^32"""
    k = lambda g: 0x400000 * (g.ny + 1) + 0x4B400000  # noqa: E731
    fast = [g for g in GEOMS if g.fast()]
    assert {g.ny for g in fast if k(g) < 1 << 32} >= {255, 256}
    assert {g.ny for g in fast if 1 << 32 <= k(g) and 0x400000 * (g.ny + 1) < 1 << 32} >= {1022}
    assert {g.ny for g in fast if 0x400000 * (g.ny + 1) >= 1 << 32} >= {1023, 1024, 4095}
    assert {g.nx for g in fast} >= set(lc.LONG)  # (the transposes: the long side in the 24-bit multiply's other operand)


@pytest.mark.parametrize("g", GEOMS, ids=IDS)
def test_host_build_of_the_header_equals_the_oracle_on_random_points(g):
    """two million points per geometry: uniform over the box grown by two cells (a quarter of them clamped into the box, so
    that the padded lookup sees its share), and one part drawn per cell next to its ties"""
    rng = np.random.default_rng(1000 + g.seed)
    n = 1 << 21
    span = lambda lim: rng.uniform(lim[0] - 2 * g.cell, lim[1] + 2 * g.cell, n).astype(f32)  # noqa: E731
    pts = np.stack([span(g.x_lim), span(g.y_lim)], 1)
    k = n // 4  # near ties: (i + 0.5 - o) * cell moved by a few ulps
    for ax, (o, m) in enumerate(((g.origin[0], g.nx), (g.origin[1], g.ny))):
        i = rng.integers(-1, m + 1, k)
        x = ((i + 0.5 - float(f32(o))) * g.cell).astype(f32)
        pts[:k, ax] = lc.ulp_step(x, rng.integers(-3, 4, k))
    pts[k:2 * k] = lc.clamp(g, pts[k:2 * k])
    for model in ("nav2d", "racing"):
        grids = g.grids()[:2 if model == "racing" else 1]
        r = emul.map_lookup(grids, g.cell, g.origin, g.x_lim, g.y_lim, pts)
        want = oracle_value(g, model, pts)
        assert np.array_equal(r["lib"].astype(np.int64), want)
        if r["usable"]:
            assert np.array_equal(r["fast"].astype(np.int64), want)
        if g.fast():
            inside = lc.in_box(g, pts)
            assert inside.sum() > n // 8
            assert np.array_equal(r["pad"][inside].astype(np.int64), want[inside])
