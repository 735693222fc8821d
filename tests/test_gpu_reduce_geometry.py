"""weights_reduce_kernel, its folds and weighted_variance_kernel on injected costs (tests/reduce_cases.py) on a real MI355X.

A generic handle of any T and dim_control samples once, hands back its clamped actions U bit for bit, takes a cost vector
written here and reduces it; the summary {min c, sum e, sum e^2, sum e*c, A[row]} and the action are held to the float64
sums of reduce_cases.reference.  u_min = 1, u_max = 3 and a mean in [1.5, 2.5] keep every action in [1, 3]: every column is
bounded away from zero and a dropped or doubled live sample moves it by at least 1 / (3 L).

Limit: TOL = 1e-5 relative on every column and every head sum, no fall-back band: the tables keep a lane's sequential fp32
chain at 80 tiles or fewer (80 * 2^-24 = 4.8e-6).  The 0 / 1 weight cases are also exact on the head sums, and the three
ways of running the reduction (regenerated noise in groups of four chains, of two chains, materialised tiles) must agree bit
for bit: same sums, same order.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reduce_cases as rc
from test_gpu_covariance import TOL, restate, weights64

pytestmark = pytest.mark.gpu

f32 = np.float32
U_MIN, U_MAX, SIGMA = 1.0, 3.0, 0.5
COV_FLOOR = 1e-6
VARIANTS = [("regen_chains4", dict(noise_regen=1, reduce_chains=4)),
            ("regen_chains2", dict(noise_regen=1, reduce_chains=2)),
            ("tiles", dict(noise_regen=0, reduce_chains=0))]
TILES_ONLY = VARIANTS[2:]
worst = {}  # table -> largest relative error seen (printed with every case)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


class Problem:
    """A generic handle that has sampled once; U[N, T, dc] are its clamped actions."""

    def __init__(self, T, dc, N, reduce_blocks=None, explore=False, covariance=False, seed=11):
        _need_gpu()
        from mppi_playground_amd import _capi

        self.T, self.dc, self.N, self.row = T, dc, N, T * dc
        f4 = C.c_float * 4
        off = 3 * N if explore else 0
        cfg = _capi.MppiConfig(model=_capi.MODEL_GENERIC, horizon=T, dim_state=2, dim_control=dc, num_samples=N,
                               sample_offset=off, inherit_count=off + (3 * N // 4 if explore else N),
                               u_min=f4(*[U_MIN] * 4), u_max=f4(*[U_MAX] * 4), sigmas=f4(*[SIGMA] * 4), seed=seed, device=0)
        self.h = h = _capi.Handle(cfg)
        if dc > _capi.MAX_DIM_CONTROL:
            fn = lambda v: (C.c_float * dc)(*[v] * dc)  # noqa: E731
            h.call("mppi_set_control_limits", fn(U_MIN), fn(U_MAX), fn(SIGMA), dc)
        if reduce_blocks is not None:
            h.call("mppi_set_option", b"reduce_blocks", reduce_blocks)
        if covariance:
            h.call("mppi_set_covariance_adaptation", 1, 1.0, COV_FLOOR, None, None)
        rng = np.random.default_rng([T, dc, N])
        self.mean = torch.from_numpy((1.5 + rng.random(self.row)).astype(f32)).cuda()
        h.call("mppi_set_mean", self.mean.data_ptr(), 1, None)
        h.call("mppi_sample", 1, None)
        U = torch.empty(N, T, dc, device="cuda")
        h.call("mppi_export_noise", None, U.data_ptr(), None)
        self.U = U.cpu().numpy()
        del U
        assert self.U.min() >= U_MIN and self.U.max() <= U_MAX
        self.summary = torch.empty(4 + self.row, device="cuda")
        self.action = torch.empty(self.row, device="cuda")
        self.stats = torch.empty(4, device="cuda")

    def load(self, costs):
        self.costs = torch.from_numpy(np.ascontiguousarray(costs, f32)).cuda()

    def reduce(self, lam, options=(), with_summary=True):
        """One reduction + finalize of the loaded costs -> (summary or None, action, finalize's head sums)."""
        h = self.h
        for key, value in dict(options).items():
            h.call("mppi_set_option", key.encode(), value)
        for buf in (self.summary, self.action, self.stats):
            buf.fill_(float("nan"))
        h.call("mppi_sample", 1, None)  # (same solve index: the same noise, materialised again where the options ask for tiles)
        h.call("mppi_set_costs", self.costs.data_ptr(), 1, None)
        h.call("mppi_weights_reduce", lam, self.summary.data_ptr() if with_summary else None, None)
        h.call("mppi_finalize", None, 1, lam, 0, self.action.data_ptr(), None, self.stats.data_ptr(), None)
        torch.cuda.synchronize()
        return (self.summary.cpu().numpy() if with_summary else None, self.action.cpu().numpy(), self.stats.cpu().numpy())

    def close(self):
        self.h.close()


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.abs(want)))


def check_reduction(table, name, p, costs, lam, live, variants):
    """Every variant's summary and action against the reference; exact head sums for 0 / 1 weights; bit-identity."""
    se, se2, sec, A = rc.reference(p.U, costs, lam)
    cmin = np.asarray(costs, f32).min()
    p.load(costs)
    outs = [p.reduce(lam, opts) for _, opts in variants]
    err = 0.0
    for (vname, _), (s, a, st) in zip(variants, outs):
        assert np.all(np.isfinite(s)) and np.all(np.isfinite(a)), f"{name} {vname}"
        e = max(_rel(s[1], se), _rel(s[2], se2), _rel(s[3], sec), _rel(s[4:], A), _rel(a.astype(np.float64) * float(s[1]), A))
        err = max(err, e)
    worst[table] = max(worst.get(table, 0.0), err)
    same = all(np.array_equal(s, outs[0][0]) and np.array_equal(a, outs[0][1]) for s, a, _ in outs)
    print(f"[reduce] {table} {name}: max rel err {err:.3e} (limit {TOL:.0e}), {len(variants)} variants "
          f"{'bit-identical' if same else 'DIFFER'}, live {len(live) if live is not None else 'dense'} of {p.N}; "
          f"table max so far {worst[table]:.3e}")
    for (vname, _), (s, a, st) in zip(variants, outs):
        assert s[0] == cmin and np.array_equal(st, s[:4]), f"{name} {vname}"
        if live is not None:
            L = len(live)
            assert s[1] == L and s[2] == L and s[3] == 8 * L and s[0] == 8, f"{name} {vname}: heads {s[:4]} for {L} live samples"
    assert err <= TOL, f"{name}: off by {err:.3e} > {TOL:.0e}"
    assert same, f"{name}: the variants' summaries or actions differ in some bit"


# ------------------------------------------------------------------------------ 1. the sample axis
@pytest.mark.parametrize("G", [g[0] for g in rc.SAMPLE_AXIS])
def test_sample_axis_geometry(G):
    _, N, rb = rc.geometry(G)
    cases = rc.sample_axis_costs(G)
    for T, dc in rc.sample_axis_rows(G):
        p = Problem(T, dc, N, reduce_blocks=rb, explore=G == rc.EXPLORE_SPLIT)
        for label, costs, lam, live in cases:
            check_reduction("sample_axis", f"{G} T{T} dc{dc} {label}", p, costs, lam, live, VARIANTS)
        p.close()


# ------------------------------------------------------------------------------ 2. the row
_ROWS = [(R, T, dc, rc.ROW_TABLE_N) for R, T, dc, _ in rc.row_table()]
_T2, _dc2, _N2 = rc.CHAINS2_BY_RULE
_ROWS.append((rc.row_shape(_T2, _dc2)[0], _T2, _dc2, _N2))


@pytest.mark.parametrize("R,T,dc,N", _ROWS, ids=[f"R{R}-T{T}-dc{dc}-N{N}" for R, T, dc, N in _ROWS])
def test_row_shapes(R, T, dc, N):
    i = _ROWS.index((R, T, dc, N))
    variants = TILES_ONLY if dc not in (1, 2, 4) else VARIANTS
    if N == _N2:  # nothing pinned: the host's own rule takes CHAINS = 2 at 300 blocks x 2 chunks
        _need_gpu()
        assert rc.blocks(N) * rc.row_shape(T, dc)[1] > 2 * torch.cuda.get_device_properties(0).multi_processor_count
        variants = [("regen_by_rule", dict(noise_regen=1, reduce_chains=0))] + VARIANTS
    p = Problem(T, dc, N)
    for label, costs, lam, live in rc.row_table_costs(i, N):
        check_reduction("row_table", f"R{R} T{T} dc{dc} N{N} {label}", p, costs, lam, live, variants)
    p.close()


# ------------------------------------------------------------------------------ 3. published rows and the folds
def test_published_row_counts_and_folds():
    """L blocks publish a partial row, L on both sides of FOLD_IN_FINALIZE_MAX_ROWS: the fold inside finalize_kernel (1),
    summarize_kernel (2) and the choice by the previous solve's row count (0, twice) against the reference and each other."""
    _, N, rb = rc.geometry(rc.FOLD_GEOMETRY)
    T, dc = 50, 2
    p = Problem(T, dc, N, reduce_blocks=rb)
    for label, costs, live in rc.fold_costs():
        se, se2, sec, A = rc.reference(p.U, costs, 1.0)
        L = len(live)
        p.load(costs)
        outs = [p.reduce(1.0, dict(fold_path=path), with_summary=False) for path in (1, 2, 0, 0)]
        err = 0.0
        for _, a, st in outs:
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(st))
            err = max(err, _rel(st[1], se), _rel(st[2], se2), _rel(st[3], sec), _rel(a, A / se))
        worst["folds"] = max(worst.get("folds", 0.0), err)
        same = all(np.array_equal(a, outs[0][1]) and np.array_equal(st, outs[0][2]) for _, a, st in outs)
        print(f"[reduce] folds {label}: max rel err {err:.3e} (limit {TOL:.0e}), {L} published rows, fold paths 1 / 2 / 0 / 0 "
              f"{'bit-identical' if same else 'DIFFER'}; table max so far {worst['folds']:.3e}")
        for _, a, st in outs:
            assert st[0] == 8 and st[1] == L and st[2] == L and st[3] == 8 * L, f"{label}: heads {st}"
        assert err <= TOL, f"{label}: off by {err:.3e} > {TOL:.0e}"
        assert same, f"{label}: the fold paths differ in some bit"
    p.close()


# ------------------------------------------------------------------------------ 4. the variance kernel
@pytest.mark.parametrize("G", rc.VARIANCE_GEOMETRIES)
def test_variance_kernel_on_the_same_geometry(G):
    """Adaptation rate 1: the table after the step is sqrt(var + floor) of this reduction's weights, whatever it held."""
    _, N, rb = rc.geometry(G)
    cases = [c for c in rc.sample_axis_costs(G, dense=("uniform",)) if c[0] in ("sparse", "uniform")]
    for T, dc in (rc.VARIANCE_ROWS[:1] if G in rc.LARGEST else rc.VARIANCE_ROWS):
        p = Problem(T, dc, N, reduce_blocks=rb, explore=G == rc.EXPLORE_SPLIT, covariance=True)
        s_old = np.full((T, dc), SIGMA, f32)
        table = torch.empty(T * dc, device="cuda")
        for label, costs, lam, live in cases:
            p.load(costs)
            h = p.h
            table.fill_(float("nan"))
            h.call("mppi_set_costs", p.costs.data_ptr(), 1, None)
            h.call("mppi_weights_reduce", lam, None, None)
            h.call("mppi_update_covariance", lam, None)
            h.call("mppi_get_sigma_table", table.data_ptr(), 1, None)
            h.call("mppi_finalize", None, 1, lam, 0, p.action.data_ptr(), None, None, None)
            torch.cuda.synchronize()
            got = table.cpu().numpy().reshape(T, dc)
            keep = np.nonzero(weights64(costs, lam)[0] != 0.0)[0]  # (samples of weight exactly 0 add nothing to any sum)
            want, var = restate(p.U[keep], np.asarray(costs, f32)[keep], lam, s_old, rate=1.0, floor=COV_FLOOR)
            err = _rel(got, want)
            worst["variance"] = max(worst.get("variance", 0.0), err)
            print(f"[reduce] variance {G} T{T} dc{dc} {label}: max rel err of s {err:.3e} (limit {TOL:.0e}), "
                  f"{len(keep)} weighted samples of {N}, s in [{want.min():.4g}, {want.max():.4g}]; "
                  f"table max so far {worst['variance']:.3e}")
            assert np.all(np.isfinite(got))
            assert err <= TOL, f"{G} T{T} dc{dc} {label}: s off by {err:.3e} > {TOL:.0e}"
        p.close()
