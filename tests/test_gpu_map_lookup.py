"""The map lookup inside the nav2d and racing cost kernels on a real MI355X, at every tie, edge and grid shape of
tests/lookup_cases.py, with no flip allowance and no margin filter.

The vehicle is held still (zero mean, zero injected noise; racing starts at speed 0), so stage 0 of every sample looks up the
start as given and every later stage looks up its clamped position — at every math level, since no sin, cos or tan result
reaches a position.  The total cost then holds value(x0) + T * value(clamp(x0)) as an integer (lookup_cases.decode), and the
oracle's rollout of the same inputs, decoded by the same rule, must give the same integer for EVERY point.  The guard
|cost - what the count stands for| < 0.5 (racing: = 0) only keeps the decoding honest.  mppi_get_math_level says which lookup
a case ran: the level the case file predicts is asserted first, so a silent fall-back to the bounds-tested kernel fails."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import lookup_cases as lc
from oracle import oracle as orc
from test_gpu_covariance import _need_gpu

pytestmark = pytest.mark.gpu

f32 = np.float32
T, N = lc.T, lc.N
MODELS = ("nav2d", "racing")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Rig:
    """One handle through the raw C ABI: zero mean, zero injected noise, horizon T, N samples."""

    def __init__(self, model, math, u_bounds=None):
        _need_gpu()
        from mppi_playground_amd import _capi

        self.model = model
        ds, dc = lc.DIMS[model]
        u_min, u_max = u_bounds or lc.U_BOUNDS[model]
        f4 = C.c_float * 4
        pad = lambda v, fill: f4(*(list(v) + [fill] * (4 - len(v))))  # noqa: E731
        cfg = _capi.MppiConfig(model=_capi.MODEL_IDS[model], horizon=T, dim_state=ds, dim_control=dc, num_samples=N,
                               sample_offset=0, inherit_count=N, u_min=pad(u_min, 0.0), u_max=pad(u_max, 0.0),
                               sigmas=pad([1.0] * dc, 0.0), seed=3, device=0)
        self.h = _capi.Handle(cfg)
        self.h.call("mppi_set_option", b"math", int(math))
        self.zero_mean, self.zero_eps = torch.zeros(T, dc, device="cuda"), torch.zeros(N, T, dc, device="cuda")
        self.h.call("mppi_set_mean", self.zero_mean.data_ptr(), 1, None)
        self.h.call("mppi_inject_noise", self.zero_eps.data_ptr(), None)

    def params(self, p):
        p = [float(v) for v in p]
        self.h.call("mppi_set_model_params", (C.c_float * len(p))(*p), len(p))

    def upload(self, slot, grid, cell, origin):
        grid = np.ascontiguousarray(grid, np.uint8)
        self.h.call("mppi_upload_map", slot, _vp(grid), grid.shape[0], grid.shape[1], float(cell), float(origin[0]), float(origin[1]))

    def reference(self, rows):
        r = np.ascontiguousarray(rows, f32)
        self.h.call("mppi_set_reference", _vp(r), r.shape[0], None)

    def setup(self, g, maps_first=False):
        """parameters, maps and (racing) the reference of geometry g, in either order"""
        steps = [lambda: self.params(lc.params(g, self.model))]
        steps += [lambda s=s, m=m: self.upload(s, *m) for s, m in enumerate(lc.maps(g, self.model))]
        for step in (steps[1:] + steps[:1]) if maps_first else steps:
            step()
        if self.model == "racing":
            self.reference(lc.reference_rows(g))
        return self

    def level(self):
        out = C.c_int(-1)
        self.h.call("mppi_get_math_level", C.byref(out))
        return out.value

    def costs(self, states):
        """[n][N] costs of the rollouts from each start state: one result tensor, one synchronisation"""
        x = torch.from_numpy(np.ascontiguousarray(states, f32)).cuda()
        out = torch.empty(len(x), N, device="cuda")
        for i in range(len(x)):
            self.h.call("mppi_set_state", x[i].data_ptr(), 1, None)
            self.h.call("mppi_rollout_cost", None)
            self.h.call("mppi_get_costs", out[i].data_ptr(), 1, None)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def particle_costs(self, states):
        """[P][N] matrix of one rollout from P start states (risk = mean)"""
        s = np.ascontiguousarray(states, f32)
        self.h.call("mppi_set_risk", 0, 1)
        self.h.call("mppi_set_particles", _vp(s), len(s), 0, None)
        x = torch.from_numpy(s[0].copy()).cuda()
        self.h.call("mppi_set_state", x.data_ptr(), 1, None)
        self.h.call("mppi_rollout_cost", None)
        out = torch.empty(len(s), N, device="cuda")
        self.h.call("mppi_get_particle_costs", out.data_ptr(), 1, None)
        torch.cuda.synchronize()
        self.h.call("mppi_set_particles", None, 0, 0, None)
        return out.cpu().numpy()

    def close(self):
        self.h.close()


# ------------------------------------------------------------------------------ the reference: the oracle's rollout, decoded
def oracle_counts(g, model, pts, maps=None, params=None):
    """the oracle's stationary rollout from every point, decoded by lookup_cases.decode (its own guard asserted)"""
    maps = lc.maps(g, model) if maps is None else maps
    params = lc.params(g, model) if params is None else params
    u_min, u_max = lc.U_BOUNDS[model]
    P = orc.Problem(model, 1, T, u_min, u_max, params=params, maps=maps, ref_path=lc.reference_rows(g) if model == "racing" else None)
    dc = lc.DIMS[model][1]
    mean, eps = np.zeros((T, dc), f32), np.zeros((1, T, dc), f32)
    costs = np.array([P.rollout_cost(s, mean, eps)["costs"][0] for s in lc.states(g, pts, model)], f32)
    k, guard = lc.decode(g, pts, costs, model)
    assert (guard == 0).all() if model == "racing" else (guard < 0.5).all()
    return k


@functools.lru_cache(maxsize=None)
def case(g, model):
    """(points, expected counts) of a geometry: computed once, shared by the three math levels, never written to"""
    pts = lc.points(g, lc.CAP)
    want = oracle_counts(g, model, pts)
    pts.setflags(write=False)
    want.setflags(write=False)
    return pts, want


def check(g, model, costs, pts, want, what=""):
    """all N costs of a point bit-identical, the guard, and the decoded count equal to the oracle's for every point"""
    costs = np.asarray(costs, f32)
    same = costs.view(np.uint32) == costs.view(np.uint32)[:, :1]
    assert same.all(), f"{g.name} {model} {what}: the samples of {int((~same.all(1)).sum())} points disagree among themselves"
    k, guard = lc.decode(g, pts, costs[:, 0], model)
    bad = np.flatnonzero(k != want)
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{g.name} {model} {what}: {len(bad)} of {len(pts)} points differ from the oracle; first: point "
                             f"{pts[i].tolist()!r} (indices {lc.indices(g, pts[i:i + 1])[0].tolist()}, in box "
                             f"{bool(lc.in_box(g, pts[i:i + 1])[0])}) gives {int(k[i])}, the oracle {int(want[i])}")
    assert (guard == 0).all() if model == "racing" else (guard < 0.5).all(), (g.name, model, what, float(guard.max()))


# ------------------------------------------------------------------------------ every geometry x model x math level
@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("g", lc.geometries(), ids=[g.name for g in lc.geometries()])
def test_every_point_decodes_to_the_oracles_count(g, model, math):
    pts, want = case(g, model)
    rig = Rig(model, math).setup(g)
    try:
        assert rig.level() == g.level(math), (g.name, model, math, "the dispatched math level is not the predicted one")
        check(g, model, rig.costs(lc.states(g, pts, model)), pts, want, f"math {math}")
    finally:
        rig.close()


# ------------------------------------------------------------------------------ the particle path
def _particle_sets(g, pts):
    """sets of 16 start positions that mix starts inside and outside the box on purpose"""
    inside = lc.in_box(g, pts)
    a, b = pts[inside], pts[~inside]
    assert len(a) >= 8 and len(b) >= 8
    sets = []
    for k in range(4):
        ia, ib = (np.arange(8) * 5 + 11 * k) % len(a), (np.arange(8) * 3 + 7 * k) % len(b)
        s = np.concatenate([a[ia], b[ib]])
        sets.append(s[np.random.default_rng(k).permutation(16)])
    sets.append(a[(np.arange(16) * 3) % len(a)])   # all inside: the copy of the loop without the bounds-tested first stage
    sets.append(b[(np.arange(16) * 3) % len(b)])
    return sets


@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["tiny-5x7-c0.3-half-exact", "long_y-3x1023-c1-last-exact", "long_x-4095x3-c0.3-half-inside"])
def test_particle_rollouts_decode_to_the_oracles_counts(name, model, math):
    g = lc.by_name(name)
    pts, _ = case(g, model)
    rig = Rig(model, math).setup(g)
    try:
        assert rig.level() == g.level(math) == math
        for s in _particle_sets(g, pts):
            check(g, model, rig.particle_costs(lc.states(g, s, model)), s, oracle_counts(g, model, s), f"particles, math {math}")
    finally:
        rig.close()


# ------------------------------------------------------------------------------ refresh_pad after every call that should
def _probes(*gs):
    """a fixed probe set: capped case points of the given geometries together (each probes the others' edges too)"""
    return np.concatenate([lc.points(g, lc.CAP)[:96] for g in gs])


def _expect(rig, g, grids, level, pts, what):
    """level and costs of the handle against the oracle on `grids` (the model's one or two [nx][ny] grids of geometry g)"""
    maps = [(grid, g.cell, g.origin) for grid in grids]
    assert rig.level() == level, (what, rig.level(), level)
    check(g, rig.model, rig.costs(lc.states(g, pts, rig.model)), pts, oracle_counts(g, rig.model, pts, maps=maps), what)


@pytest.mark.parametrize("math", [1, 2])
@pytest.mark.parametrize("model", MODELS)
def test_the_padded_grid_follows_every_call_that_changes_it(model, math):
    g = lc.by_name("tiny-5x7-c0.3-half-exact")
    big = lc.by_name("long_y-3x1023-c1-last-exact")
    small = lc.by_name("tiny-1x7-c0.05-last-exact")
    racing = model == "racing"
    a, b, b2 = g.grids()
    pts = _probes(g)
    first = Rig(model, math).setup(g, maps_first=True)            # 1. maps, then parameters
    rig = Rig(model, math).setup(g)                               # 2. parameters, then maps
    clone = Rig(model, math)
    try:
        _expect(first, g, (a, b)[:1 + racing], math, pts, "maps before parameters")
        _expect(rig, g, (a, b)[:1 + racing], math, pts, "parameters before maps")
        if racing:
            rig.upload(1, b2, g.cell, g.origin)                   # 3. only the lane grid: the summed pad must change
            assert (b2 != b).any()
            _expect(rig, g, (a, b2), math, pts, "another lane grid")
            # 4. slot 0 of another geometry (inside the old limits' reach or not: the oracle takes each grid's own geometry)
            other = dataclasses.replace(g, nx=7, ny=5, origin=(g.origin[1], g.origin[0]))
            a_other = other.grids()[0]
            maps = [(a_other, other.cell, other.origin), (b2, g.cell, g.origin)]
            rig.upload(0, a_other, other.cell, other.origin)
            assert rig.level() == 0, "racing maps of two geometries cannot share a padded grid"
            check(g, model, rig.costs(lc.states(g, pts, model)), pts, oracle_counts(g, model, pts, maps=maps), "two geometries")
            rig.upload(0, a, g.cell, g.origin)                    # 5. back in line
            _expect(rig, g, (a, b2), math, pts, "geometries in line again")
        for h, what in ((big, "a larger map (the pad is reallocated)"), (small, "a smaller map (the pad buffer is reused)")):
            rig.params(lc.params(h, model))                       # 6. / 7. (limits first: no map is ever left outside its plan)
            for slot, m in enumerate(lc.maps(h, model)):
                rig.upload(slot, *m)
            if racing:
                rig.reference(lc.reference_rows(h))
            _expect(rig, h, h.grids()[:1 + racing], math, _probes(h, g), what)
        wide = dataclasses.replace(small, x_lim=(small.x_lim[0] - 2 * small.cell, small.x_lim[1] + 2 * small.cell))
        rig.params(lc.params(wide, model))                        # 8. limits beyond the pad, and back
        assert not wide.fast()
        _expect(rig, wide, small.grids()[:1 + racing], 0, _probes(wide), "limits widened beyond the padded grid")
        rig.params(lc.params(small, model))
        _expect(rig, small, small.grids()[:1 + racing], math, _probes(small), "limits narrowed back")
        # 9. a map rasterised on the device, on a stream of the caller's
        rig.params(lc.params(g, model))
        for slot, m in enumerate(lc.maps(g, model)):
            rig.upload(slot, *m)
        if racing:
            rig.reference(lc.reference_rows(g))
        side = torch.cuda.Stream()
        circles, rects = np.array([[1, 2, 1], [4, 6, 0]], np.int32), np.array([[0, 4, 1, 6]], np.int32)
        rig.h.call("mppi_build_obstacle_map", 0, g.nx, g.ny, g.cell, g.origin[0], g.origin[1], _vp(circles), len(circles),
                   _vp(rects), len(rects), C.c_void_p(side.cuda_stream))
        built = np.zeros((g.nx, g.ny), np.uint8)
        rig.h.call("mppi_download_map", 0, _vp(built), None, None)
        assert 0 < built.sum() < built.size and (built != a).any()
        _expect(rig, g, (built, b)[:1 + racing], math, pts, "a map built on a side stream")
        # 10. a clone answers from its own maps after the source's change
        clone.h.call("mppi_clone_state", rig.h.h)
        rig.upload(0, 1 - built, g.cell, g.origin)
        _expect(clone, g, (built, b)[:1 + racing], math, pts, "the clone, after the source changed its map")
        _expect(rig, g, (1 - built, b)[:1 + racing], math, pts, "the source of the clone")
    finally:
        for r in (first, rig, clone):
            r.close()


# ------------------------------------------------------------------------------ the gate's truth table
def _gate(rig, g, pts, want, params, level, what):
    rig.params(params)
    assert rig.level() == level, (what, rig.level(), level)
    check(g, rig.model, rig.costs(lc.states(g, pts, rig.model)), pts, want, what)


@pytest.mark.parametrize("math", [1, 2])
def test_gate_nav2d(math):
    g = lc.by_name("tiny-5x7-c0.3-half-exact")
    pts, want = case(g, "nav2d")
    rig = Rig("nav2d", math).setup(g)
    try:
        base = lc.params(g, "nav2d")  # {vmin, vmax, wmin, wmax, dt, ...}; the solver's bounds are (0, -1) .. (2, 1)
        edit = lambda **kw: [kw.get(k, v) for k, v in zip(("vmin", "vmax", "wmin", "wmax", "dt"), base)] + base[5:]  # noqa: E731
        under3 = float(np.nextafter(f32(3.0), f32(0)))
        for params, level, what in [
                (base, math, "the shipped clamp"),
                (edit(vmax=1.5), 0, "solver bounds wider than the model's speed clamp"),
                (base, math, "and back"),
                (edit(wmin=-0.5), 0, "solver bounds wider than the model's turn-rate clamp"),
                (edit(wmin=-3.0, wmax=3.0, dt=1.0), 0, "|w|max * dt = 3"),
                (edit(wmin=-under3, wmax=under3, dt=1.0), math, "|w|max * dt just under 3"),
                (edit(wmin=-1.0, wmax=6.0, dt=0.5), 0, "|w|max * dt = 3 from the upper bound"),
                (base, math, "and back again")]:
            _gate(rig, g, pts, want, params, level, what)
    finally:
        rig.close()


@pytest.mark.parametrize("math", [1, 2])
def test_gate_racing(math):
    g = lc.by_name("tiny-5x7-c0.3-half-exact")
    pts, want = case(g, "racing")
    rig = Rig("racing", math).setup(g)
    try:
        over = float(np.nextafter(f32(0.25), f32(1)))
        ones_L = float(np.nextafter(f32(2.0), f32(0)))
        p = lambda **kw: lc.racing_params(g, **kw)  # noqa: E731  (the solver's bounds are (-2, -0.25) .. (2, 0.25))
        for params, level, what in [
                (p(), math, "steer 0.25, L = 1"),
                (p(u_max=(1.5, 0.25)), 0, "solver bounds wider than the model's acceleration clamp"),
                (p(), math, "and back"),
                (p(u_min=(-2.0, -over), u_max=(2.0, over)), 0, "steer just above 0.25: no polynomial tangent"),
                (p(u_min=(-2.0, -over)), 0, "the lower steer bound alone"),
                (p(L=2.5), math, "a generic wheel base"),
                (p(L=ones_L), 0, "a wheel base with an all-ones significand"),
                (p(L=1.0), math, "L = 1 again")]:
            _gate(rig, g, pts, want, params, level, what)
    finally:
        rig.close()
