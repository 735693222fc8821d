"""The softmax statistics under every automatic temperature rule — stats_partial_kernel + stats_combine_kernel (one
temperature) and stats_multi_block + stats_combine_columns (32 temperatures) — on injected costs (tests/stats_cases.py) on a
real MI355X, and the searches that stand on them.

A generic handle of N samples takes a cost vector written here (mppi_set_costs) and reduces it.  Exact cases: one cost of weight
1 at every edge of the launch geometry, all of them at once, equal costs, and the minimum / maximum at those edges.  Dense cases:
sum e, sum e^2 (relative to themselves) and sum e*c (relative to sum e*|c|) against float64 sums over the argument each kernel
forms in fp32.  Limit: max(1e-5, chain * 2^-24), which the tables keep at 1e-5 everywhere; no fall-back band.  (sum e*c is
allowed 2^-149 * (sum |c| + N) absolute on top, stats_cases.underflow_floor: where every cost of normal weight is 0 the sum is
made of denormal weights alone — 2e-42 at N = 257 — which fp32 holds to 2^-149, not to 2^-24 relative.)

On top of the sums: the ESSPS chain against its host loop and against ESS in float64, the LBPS grid search against a twin that
steps lbps_grid_step on the host over the device's own sums (1e-12: the same sums, correctly rounded operations), the Brent
search against its host loop to the bit, and mpo_step_kernel against mpo_step on the host from the device's statistics (4 fp32
ulp).  Every test only feeds costs and reads sums or temperatures.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import emul
import stats_cases as sc
from helpers import same_lbps_minimum

pytestmark = pytest.mark.gpu

f32 = np.float32
worst = {}  # table -> (largest error seen, where)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _note(table, err, where):
    if err >= worst.get(table, (-1.0, ""))[0]:
        worst[table] = (err, where)


def _report(table, unit=""):
    err, where = worst.get(table, (0.0, "-"))
    print(f"[stats] {table}: largest so far {err:.3e}{unit} at {where}")


class Stats:
    """A generic handle of N samples (T = 1, one control) that has sampled once; costs come from `load` / `push`."""

    def __init__(self, N):
        _need_gpu()
        from mppi_playground_amd import _capi

        self.N = N
        f4 = C.c_float * 4
        cfg = _capi.MppiConfig(model=_capi.MODEL_GENERIC, horizon=1, dim_state=2, dim_control=1, num_samples=N, sample_offset=0,
                               inherit_count=N, u_min=f4(*[1.0] * 4), u_max=f4(*[3.0] * 4), sigmas=f4(*[0.5] * 4), seed=11, device=0)
        self.h = h = _capi.Handle(cfg)
        self.mean = torch.full((1,), 2.0, device="cuda")
        h.call("mppi_set_mean", self.mean.data_ptr(), 1, None)
        h.call("mppi_sample", 1, None)
        self.cd = None

    def load(self, costs):
        self.cd = torch.from_numpy(np.ascontiguousarray(costs, f32)).cuda()
        self.push()

    def push(self):
        """(again after `cd` was changed in place)"""
        self.h.call("mppi_set_costs", self.cd.data_ptr(), 1, None)

    def one(self, lam):
        """mppi_softmax_stats -> [cmin, cmax, sum e, sum e^2, sum e*c]"""
        out = (C.c_double * 5)(*[float("nan")] * 5)
        self.h.call("mppi_softmax_stats", C.c_float(float(lam)), out, None)
        return list(out)

    def multi(self, lams):
        """mppi_softmax_stats_multi -> [len(lams)][3]"""
        lams = np.ascontiguousarray(lams, f32)
        n = len(lams)
        out = (C.c_double * 96)(*[float("nan")] * 96)
        self.h.call("mppi_softmax_stats_multi", lams.ctypes.data_as(C.c_void_p), n, out, None)
        assert all(np.isnan(v) for v in out[3 * n:])
        return np.array(out[:3 * n], np.float64).reshape(n, 3)

    def get_lambda(self):
        lam = C.c_double(float("nan"))
        self.h.call("mppi_get_lambda", C.byref(lam), None, None)
        return lam.value

    def close(self):
        self.h.close()


# ------------------------------------------------------------------------------ 1. exact cases
@pytest.mark.parametrize("N", sc.ALL_SIZES)
def test_exact_sums_and_extremes_at_every_edge(N):
    s = Stats(N)
    pos = sc.positions(N)
    host = np.full(N, sc.DEAD, f32)
    s.cd = torch.from_numpy(host).cuda()

    def check(live, tag):
        L = len(live)
        s.push()
        for lam in sc.EXACT_LAMBDAS:
            o = s.one(lam)
            assert o == [host.min(), host.max(), L, L, sc.LIVE * L], f"N {N} {tag} lambda {lam}: one temperature {o}"
        m = s.multi(sc.SET_SHUFFLED)
        assert np.array_equal(m, np.tile([L, L, sc.LIVE * L], (32, 1))), f"N {N} {tag}: 32 temperatures {m.tolist()}"

    for p in pos:                       # one live cost at p alone
        host[p] = sc.LIVE
        s.cd[p] = sc.LIVE
        check([p], f"one live cost at {p}")
        host[p] = sc.DEAD
        s.cd[p] = sc.DEAD
    idx = torch.tensor(pos, device="cuda")
    host[pos] = sc.LIVE
    s.cd[idx] = sc.LIVE
    check(pos, "all positions live")
    host[:] = sc.EQUAL                  # all equal
    s.cd.fill_(sc.EQUAL)
    s.push()
    want = [N, N, sc.EQUAL * N]
    for lam in sc.EXACT_LAMBDAS:
        o = s.one(lam)
        assert o == [sc.EQUAL, sc.EQUAL] + want, f"N {N} all equal lambda {lam}: {o}"
    m = s.multi(sc.SET_SHUFFLED)
    assert np.array_equal(m, np.tile(want, (32, 1))), f"N {N} all equal: {m.tolist()}"
    host[:] = sc.PLATEAU                # the maximum, then the minimum, at p (min_cost_kernel and both kernels' maxima)
    s.cd.fill_(sc.PLATEAU)
    for p in pos:
        for value in (sc.PEAK, sc.PIT):
            host[p] = value
            s.cd[p] = value
            s.push()
            o = s.one(1.0)
            assert o[0] == host.min() and o[1] == host.max(), f"N {N} {value} at {p}: cmin {o[0]} cmax {o[1]}"
        host[p] = sc.PLATEAU
        s.cd[p] = sc.PLATEAU
    print(f"[stats] exact N {N}: {len(pos)} positions {pos}, one / all live, equal costs, extremes: exact")
    s.close()


# ------------------------------------------------------------------------------ 2. dense cases
@pytest.mark.parametrize("N", sc.ONE_SIZES)
def test_dense_sums_one_temperature(N):
    s = Stats(N)
    lim = sc.limit(sc.chain_one(N))
    for kind in sc.DENSE_KINDS:
        c = sc.dense_costs(N, kind)
        ref = sc.reference_one(c, sc.ONE_LAMBDAS)
        floor = sc.underflow_floor(c)
        s.load(c)
        for j, lam in enumerate(sc.ONE_LAMBDAS):
            o = s.one(lam)
            err = sc.sums_error(o[2:], ref[j], floor)
            _note("one_temperature", err, f"N {N} {kind} lambda {lam:.4g}")
            assert o[0] == c.min() and o[1] == c.max(), (N, kind, o[:2])
            assert err <= lim, f"N {N} {kind} lambda {lam}: off by {err:.3e} > {lim:.0e} ({o[2:]} against {ref[j].tolist()})"
    _report("one_temperature")
    s.close()


@pytest.mark.parametrize("N", sc.MULTI_SIZES)
def test_dense_sums_32_temperatures_and_unused_slots(N):
    s = Stats(N)
    lim = sc.limit(sc.chain_multi(N))
    perm = (13 * np.arange(32) + 5) % 32
    for kind in sc.DENSE_KINDS:
        c = sc.dense_costs(N, kind)
        narrow, wide = sc.reference_multi(c, sc.SET_NARROW), sc.reference_multi(c, sc.SET_WIDE)
        refs = {"narrow": narrow, "count31": narrow[:31], "count1": narrow[:1], "wide": wide, "shuffled": wide[perm]}
        floor = sc.underflow_floor(c)
        s.load(c)
        got = {}
        for name in ("narrow", "count31", "count1", "wide", "shuffled"):  # (the short counts right after a count-32 call)
            got[name] = s.multi(sc.TEMPERATURE_SETS[name])
            err = sc.sums_error(got[name], refs[name], floor)
            _note("32_temperatures", err, f"N {N} {kind} {name}")
            assert err <= lim, f"N {N} {kind} {name}: off by {err:.3e} > {lim:.0e}"
        assert np.array_equal(got["count31"], got["narrow"][:31]) and np.array_equal(got["count1"], got["narrow"][:1]), (N, kind)
        assert np.array_equal(got["shuffled"], got["wide"][perm]), (N, kind)  # a column does not depend on its slot
    _report("32_temperatures")
    s.close()


# ------------------------------------------------------------------------------ 3. the ESSPS chain
@pytest.mark.parametrize("N", sc.SEARCH_SIZES)
def test_essps_chain_against_host_loop_and_float64(N):
    s = Stats(N)
    h = s.h
    lo, hi = sc.LAM_MIN, sc.LAM_MAX
    for kind in sc.ESSPS_SHAPES:
        c = sc.dense_costs(N, kind)
        s.load(c)
        ess = {}

        def check64(lam, target, end, tag):
            if end is not None:
                assert lam == end, f"{tag}: {lam} where float64 decides the end point {end}"
                return
            if lam not in ess:
                ess[lam] = sc.ess64(c, lam)
            off = abs(ess[lam] - target) / target
            _note("essps_ess64", off, tag)
            assert lo < lam < hi and off <= sc.ESS_BAND, f"{tag}: ESS64({lam}) = {ess[lam]} for target {target}: off by {off:.3e}"

        for target in sc.essps_targets(N):
            end = sc.essps_end_point(c, target, lo, hi)
            for merge0 in (0, 1):
                tag = f"N {N} {kind} target {target:g} merge0 {merge0}"
                h.call("mppi_set_option", b"essps_merge0", merge0)
                h.call("mppi_set_option", b"essps_cold", 1)
                lam_host = C.c_double(0.0)
                h.call("mppi_essps_lambda", float(target), lo, hi, C.byref(lam_host), None)
                h.call("mppi_essps_lambda_device", float(target), lo, hi, None)
                cold = s.get_lambda()
                err = abs(cold - lam_host.value) / lam_host.value
                _note("essps_cold_vs_host", err, tag)
                assert err <= sc.COLD_TOL, f"{tag}: cold {cold} host {lam_host.value}"
                check64(cold, target, end, tag + " cold")
                for k in range(2):
                    h.call("mppi_essps_lambda_device", float(target), lo, hi, None)
                    warm = s.get_lambda()
                    err = abs(warm - lam_host.value) / lam_host.value
                    _note("essps_warm_vs_host", err, tag)
                    assert err <= sc.WARM_TOL, f"{tag}: warm {k} {warm} host {lam_host.value}"
                    check64(warm, target, end, tag + f" warm {k}")
    h.call("mppi_set_option", b"essps_merge0", 0)
    for t in ("essps_cold_vs_host", "essps_warm_vs_host", "essps_ess64"):
        _report(t)
    s.close()


# ------------------------------------------------------------------------------ 4. the LBPS grid search and its twin
def lbps_twin(s, delta):
    """lbps_select_kernel's rounds on the host: the device's sums per grid, the objective and the grid step in float64."""
    lo, hi = sc.LAM_MIN, sc.LAM_MAX
    cmin, cmax = s.one(1.0)[:2]
    lam = float("nan")
    for r in range(sc.LBPS_GRID_ROUNDS):
        grid = [sc.grid_point(lo, hi, j) for j in range(32)]
        sums = s.multi(np.asarray(grid, np.float64).astype(f32))
        obj = [sc.lbps_objective(cmin, cmax, se, se2, sec, delta) for se, se2, sec in sums]
        lo, hi, lam = emul.lbps_grid_step(grid, obj, r == sc.LBPS_GRID_ROUNDS - 1)
    return lam


@pytest.mark.parametrize("N", sc.SEARCH_SIZES)
def test_lbps_grid_search_against_its_host_twin(N):
    s = Stats(N)
    emul.search_lib()
    dense = [(k, sc.dense_costs(N, k)) for k in sc.DENSE_KINDS[:sc.BRENT_KINDS]]
    pos = sc.positions(N)
    peaks = [(f"max_at_{p}", sc.extreme_at(N, p, sc.PEAK)) for p in pos]
    raised = [(f"raised_at_{p}", sc.raised_max_at(N, p)) for p in pos]   # (a dense objective that the cost range shapes)
    # float64 sums do not depend on where the maximum sits: one float64 search serves every vector of either family
    jobs = [(c, d) for _, c in dense + peaks[:1] + raised[:1] for d in sc.LBPS_DELTAS]
    f64 = sc.pmap(lambda a: emul.lbps_grid(a[0], a[1], sc.LAM_MIN, sc.LAM_MAX), jobs)
    which = list(range(len(dense))) + [len(dense)] * len(peaks) + [len(dense) + 1] * len(raised)
    for i, (label, c) in enumerate(dense + peaks + raised):
        s.load(c)
        for k, delta in enumerate(sc.LBPS_DELTAS):
            tag = f"N {N} {label} delta {delta}"
            s.h.call("mppi_lbps_lambda_device", delta, sc.LAM_MIN, sc.LAM_MAX, None)
            lam = s.get_lambda()
            twin = lbps_twin(s, delta)
            err = abs(lam - twin) / twin
            _note("lbps_grid_vs_twin", err, tag)
            assert err <= sc.TWIN_TOL, f"{tag}: device {lam!r} twin {twin!r}"
            want = f64[2 * which[i] + k]
            # (a plateau of minimisers — see test_lbps_grid_reference_meets_its_band_alone — has no point to agree on)
            same = same_lbps_minimum(c, lam, want, delta=delta) or (label.startswith(sc.PLATEAU_KINDS) and sc.on_one_plateau(c, lam, want, delta))
            assert same, f"{tag}: device {lam} float64 {want}"
    _report("lbps_grid_vs_twin")
    s.close()


# ------------------------------------------------------------------------------ 5. the Brent search on the verified sums
@pytest.mark.parametrize("N", sc.ONE_SIZES)
def test_brent_search_equals_its_host_loop_at_every_group_count(N):
    """lbps_brent_kernel repeats stats_partial_thread probe for probe over 1 .. 4 groups of virtual blocks: the temperature of
    the host loop over mppi_softmax_stats (whose sums the dense test holds to float64) to the bit, staged in LDS or not."""
    s = Stats(N)
    emul.search_lib()
    small = N <= 65791   # (a float64 search costs ~30 passes over the costs on the host)
    vecs = [sc.dense_costs(N, k) for k in sc.DENSE_KINDS[:sc.BRENT_KINDS]]
    f64 = sc.pmap(lambda c: emul.lbps(c, 0.01, sc.LAM_MIN, sc.LAM_MAX)[0], vecs) if small else None
    for i, c in enumerate(vecs):
        s.load(c)
        lam_host = C.c_double(0.0)
        s.h.call("mppi_lbps_lambda", 0.01, sc.LAM_MIN, sc.LAM_MAX, C.byref(lam_host), None)
        s.h.call("mppi_lbps_brent_device", 0.01, sc.LAM_MIN, sc.LAM_MAX, None)
        lam = s.get_lambda()
        assert not s.h.lib.mppi_search_error(s.h.h)
        assert lam == lam_host.value, f"N {N} brent{i}: device {lam!r} host loop {lam_host.value!r}"
        if small:
            assert same_lbps_minimum(c, lam, f64[i]), f"N {N} brent{i}: device {lam} float64 {f64[i]}"
    s.close()


# ------------------------------------------------------------------------------ 6. the MPO step
@pytest.mark.parametrize("N", sc.MPO_SIZES)
def test_mpo_step_against_the_host_step_on_the_device_statistics(N):
    s = Stats(N)
    emul.search_lib()
    epsilon, lr = 0.1, 0.2
    st4 = (C.c_double * 4)()

    def state():
        s.h.call("mppi_mpo_state", st4)
        return np.array(list(st4), np.float64)

    for kind in (0, 1):   # nav2d-like and racing-like: |c| / T is large, the two halves of the gradient cancel
        rng = np.random.default_rng([21, N, kind])
        s.h.call("mppi_mpo_reset", 1.0, epsilon, lr)
        for step in range(4):
            c = sc.brent_cost_vector(rng, N, kind)
            s.load(c)
            before = state()
            stats = s.one(sc.softplus32(before[0]))
            want, lam_want = emul.mpo_step_stats(before, epsilon, lr, stats)
            lam = C.c_double(0.0)
            s.h.call("mppi_mpo_step", C.byref(lam), None)
            got = state()
            ulp = max(sc.ulp32(got[i], want[i]) for i in range(3))
            tag = f"N {N} kind {kind} step {step}"
            _note("mpo_ulp", ulp, tag)
            assert got[3] == want[3] == step + 1, (tag, got, want)
            assert ulp <= sc.MPO_ULP, f"{tag}: {{log T, m, v}} {got[:3].tolist()} against {want[:3].tolist()}: {ulp} ulp"
            # (exp of an fp32 log T that may differ by 4 ulp, |log T| < 7, and of another fp32 exp: 4 * 2^-24 * 7 + 2^-23)
            assert abs(lam.value - lam_want) <= 2e-6 * lam_want, (tag, lam.value, lam_want)
    _report("mpo_ulp", " ulp")
    s.close()
