"""solve_fused_kernel (mppi_solve as ONE cooperative launch) at every block geometry (tests/fused_cases.py) on a real MI355X.

The kernel cannot take injected costs, so the cases choose what the costs ARE: a scout handle of 3N samples rolls out from the
same seed and state, and a fresh N-sample handle whose sample_offset slides its window over the scout's samples puts the
scout's cheapest sample at any local index; a temperature of gap / 110 leaves that sample with weight exactly 1 and every other
with exactly 0, lambda = 1e30 gives every sample weight exactly 1, and the standard deviation of the costs gives dense
weights, which are held to the float64 sums of fused_cases.reference on the device's own costs and exported actions.

Every case asks the library which geometry the solve took (mppi_fused_geometry) and holds it to fused_cases.geometry for
this device's compute-unit count: no case can pass on the multi-kernel path.

Limit of the dense cases: max(TOL, chain * 2^-24) with TOL = 1e-5 and `chain` the longest sequential fp32 addition chain of
a column through the kernel (fused_cases.chain), relative to the column's scale sum w |U| (sum e |c| for sum e*c): the
native models' actions are signed.  No fall-back band.  The placed and the all-equal cases are exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_cases as fc
from helpers import MODEL_CFG, oracle_problem, rel_err, same_lbps_minimum
from test_gpu_covariance import TOL, make, weights64

pytestmark = pytest.mark.gpu

f32 = np.float32
ALL_INHERIT = 1 << 40   # inherit_count of a window handle: every sample inherits the warm start, whatever its global index
worst = {}              # table -> largest error seen (printed with every case)


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def took(h):
    """(blocks, spb) of the handle's last mppi_solve: (0, 0) for the multi-kernel path."""
    g, s = C.c_int(-1), C.c_int(-1)
    h.call("mppi_fused_geometry", C.byref(g), C.byref(s))
    return g.value, s.value


def assert_single_launch(h, N, name, **kw):
    """The last solve was the single launch with the geometry the table was written for; -> (G, spb)."""
    want = fc.geometry(N, _cu(), **kw)
    assert want is not None, f"{name}: the table expects a single launch on {_cu()} compute units"
    assert took(h) == want, f"{name}: took {took(h)}, the case was written for {want}"
    assert h.lib.mppi_fused_error(h.h) == 0, name
    return want


class Raw:
    """A native-model handle driven through the C ABI: its own window [offset, offset + N) of the seed's sample stream."""

    def __init__(self, model, T, N, offset=0, inherit=None, mode=None, exploration=0.0):
        self.model, self.T, self.N = model, T, N
        self.solver, x0 = make(model, T, N, 1.0, **(dict(exploration=exploration) if exploration else {}))
        self.dc = self.solver._dim_control
        self.ds = self.solver._dim_state
        self.x0 = x0.to("cuda", torch.float32).contiguous()
        self.action = torch.empty(T, self.dc, device="cuda")
        self.state = torch.empty(1, T + 1, self.ds, device="cuda")
        self.stats = torch.empty(4, device="cuda")
        self.mode = mode
        self._prepare()
        if offset or inherit is not None:
            self.window(offset, inherit)

    @property
    def h(self):
        return self.solver._h

    def _prepare(self):
        self.solver._refresh_model_inputs()   # (maps and parameters of the model: forward() is never called here)
        if self.mode is not None:
            self.h.call("mppi_set_option", b"fused_solve", self.mode)
        self.h.call("mppi_set_state", self.x0.data_ptr(), 1, self.solver._stream())

    def window(self, offset, inherit=None):
        """Re-create the handle as the N samples from global index `offset` on (like a shard of a larger problem)."""
        from mppi_playground_amd import _capi

        sol = self.solver
        cfg = _capi.MppiConfig()
        cfg.model = _capi.MODEL_IDS[self.model]
        cfg.horizon, cfg.dim_state, cfg.dim_control = self.T, self.ds, self.dc
        cfg.num_samples, cfg.sample_offset = self.N, int(offset)
        cfg.inherit_count = ALL_INHERIT if inherit is None else int(inherit)
        for k in range(self.dc):
            cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = (MODEL_CFG[self.model][q][k] for q in ("u_min", "u_max", "sigmas"))
        cfg.seed, cfg.device = sol._seed, 0
        sol._h.close()
        sol._h = _capi.Handle(cfg)
        sol._uploaded, sol._params_set, sol._ref_uploaded = {}, None, None
        self._prepare()

    def set_mean(self, mean):
        self._mean = torch.from_numpy(np.ascontiguousarray(mean, f32).reshape(self.T, self.dc)).cuda()
        self.h.call("mppi_set_mean", self._mean.data_ptr(), 1, self.solver._stream())

    def mean(self):
        m = torch.empty(self.T, self.dc, device="cuda")
        self.h.call("mppi_get_mean", m.data_ptr(), 1, self.solver._stream())
        return m.cpu().numpy()

    def costs(self):
        c = torch.empty(self.N, device="cuda")
        self.h.call("mppi_get_costs", c.data_ptr(), 1, self.solver._stream())
        return c.cpu().numpy()

    def rollout(self, idx):
        """Costs of solve index `idx` around the current mean by the multi-kernel path's rollout kernel (no solve)."""
        st = self.solver._stream()
        self.h.call("mppi_sample", idx, st)
        self.h.call("mppi_rollout_cost", st)
        return self.costs()

    def solve(self, idx, lam):
        """One mppi_solve -> (action [T, dc], state sequence [T + 1, ds], {c_min, sum e, sum e^2, sum e*c}, costs [N])."""
        for buf in (self.action, self.state, self.stats):
            buf.fill_(float("nan"))
        self.h.call("mppi_solve", None, idx, float(lam), self.action.data_ptr(), self.state.data_ptr(), self.stats.data_ptr(),
                    self.solver._stream())
        torch.cuda.synchronize()
        return self.action.cpu().numpy(), self.state.cpu().numpy()[0], self.stats.cpu().numpy(), self.costs()

    def actions_around(self, mean):
        """U[N, T, dc] = clamp(mean + eps) of the last solve's noise; the stored warm start is put back."""
        st = self.solver._stream()
        keep = self.mean()
        self.set_mean(mean)
        U = torch.empty(self.N, self.T, self.dc, device="cuda")
        self.h.call("mppi_export_noise", None, U.data_ptr(), st)
        out = U.cpu().numpy()
        self.set_mean(keep)
        return out

    def close(self):
        self.solver._h.close()


def _size_case(N):
    mode = fc.fused_mode(N)
    return mode, dict(mode=mode, row=fc.SIZE_T)


# ------------------------------------------------------------------------------ (a) one weighted sample, placed
def find_winner(scout, N):
    """(solve index, costs[3N], g*, gap): the first solve index whose cheapest sample of 3N lies in the middle third, alone
    at the minimum, with a gap that lambda = gap / 110 resolves: |c| / lambda < 1e7 keeps the rounding of the two fp32 quotients
    of the weight argument below 1.2, i.e. every other argument below -108 and its expf at exactly 0."""
    why = []
    for idx in range(1, 21):
        c = scout.rollout(idx)
        g = int(np.argmin(c))
        two = np.partition(c.astype(np.float64), 1)[:2] if len(c) > 1 else np.array([c[0], np.inf])
        gap = float(two[1] - two[0])
        if N <= g < 2 * N and gap > 0.0 and 110.0 * float(np.abs(c).max()) / gap < 1e7:
            return idx, c, g, gap
        why.append((idx, g, gap))
    pytest.fail(f"N = {N}: no solve index in 1..20 puts a lone, resolvable minimum into [N, 2N): {why}")


@pytest.mark.parametrize("N", fc.SIZE_NS)
def test_one_weighted_sample_at_every_edge(N):
    T = fc.SIZE_T
    mode, kw = _size_case(N)
    scout = Raw("pendulum", T, 3 * N, inherit=ALL_INHERIT, mode=0)
    scout.set_mean(np.zeros(T))
    idx, c3, g, gap = find_winner(scout, N)
    x0 = scout.x0.cpu().numpy()
    scout.close()
    lam = gap / 110.0
    P = oracle_problem("pendulum", 1, T)
    p = Raw("pendulum", T, N, mode=mode)
    G, spb = fc.geometry(N, _cu(), **kw)
    places = fc.targets(N, G, spb)
    for i in places:
        name = f"N{N} winner at {i} (block {i // spb}, thread {i % spb})"
        p.window(g - i)
        p.set_mean(np.zeros(T))
        a, s, st, c = p.solve(idx, lam)
        assert_single_launch(p.h, N, name, **kw)
        warm = p.mean()
        U = p.actions_around(np.zeros(T))
        assert np.array_equal(c, c3[g - i:g - i + N]), f"{name}: costs differ from the scout's window"
        assert int(np.argmin(c)) == i and st[0] == c3[g], name
        assert st[1] == 1.0 and st[2] == 1.0 and st[3] == c3[g], f"{name}: heads {st}"
        assert np.array_equal(a, U[i]), f"{name}: action\n{a.ravel()}\nwinner's row\n{U[i].ravel()}"
        assert np.array_equal(warm, a), name
        assert rel_err(s, P.rollout_single(x0, a)) < TOL, name
    print(f"[fused] placed N{N} G{G} spb{spb}: {len(places)} places {places}, solve index {idx}, gap {gap:.3e}, "
          f"max |c| / lambda {float(np.abs(c3).max()) / lam:.3e}: all exact")
    p.close()


# ------------------------------------------------------------------------------ (b) all weights equal
@pytest.mark.parametrize("N", fc.SIZE_NS)
def test_equal_weights_count_every_lane(N):
    T = fc.SIZE_T
    mode, kw = _size_case(N)
    p = Raw("pendulum", T, N, mode=mode)
    p.set_mean(np.zeros(T))
    a, s, st, c = p.solve(1, 1e30)
    G, spb = assert_single_launch(p.h, N, f"N{N}", **kw)
    U = p.actions_around(np.zeros(T)).reshape(N, -1).astype(np.float64)
    lim = fc.limit(G, spb, fc.row_shape(T, 1)[0], TOL)
    c64 = c.astype(np.float64)
    err_c = abs(float(st[3]) - c64.sum()) / np.abs(c64).sum()
    err_a = float(np.max(np.abs(a.ravel().astype(np.float64) - U.mean(0)) / np.abs(U).mean(0)))
    err = max(err_c, err_a)
    worst["equal"] = max(worst.get("equal", 0.0), err)
    print(f"[fused] equal N{N} G{G} spb{spb}: sum e {st[1]:.1f}, sum e^2 {st[2]:.1f}, err of sum e*c {err_c:.3e}, of the mean "
          f"action {err_a:.3e} (limit {lim:.3e}); table max so far {worst['equal']:.3e}")
    assert st[0] == c.min() and st[1] == N and st[2] == N, f"N{N}: heads {st}"
    assert err <= lim, f"N{N}: off by {err:.3e} > {lim:.3e}"
    p.close()


# ------------------------------------------------------------------------------ (c) dense weights
def check_dense(table, name, p, idx, lam, mean_used, **kw):
    """One solve at `lam`; heads and every action column against the float64 reference on the device's costs and actions."""
    a, s, st, c = p.solve(idx, lam)
    G, spb = assert_single_launch(p.h, p.N, name, **kw)
    st = st.astype(np.float64)   # (the fp32 heads, exactly: a float32 minus a Python float would round the reference first)
    U = p.actions_around(mean_used)
    cmin, se, se2, sec, A = fc.reference(U, c, lam, G, spb)
    e = fc.weights(c, lam, G, spb)
    sc, S = fc.scales(U, c, e)
    lim = fc.limit(G, spb, fc.row_shape(p.T, p.dc)[0], TOL)
    errs = dict(se=abs(st[1] - se) / se, se2=abs(st[2] - se2) / se2, sec=abs(st[3] - sec) / sc,
                action=float(np.max(np.abs(a.ravel().astype(np.float64) - A / se) / (S / se))))
    err = max(errs.values())
    worst[table] = max(worst.get(table, 0.0), err)
    print(f"[fused] {table} {name} G{G} spb{spb}: max err {err:.3e} (limit {lim:.3e}; "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"), ESS {se * se / se2:.1f} of {p.N}; "
          f"table max so far {worst[table]:.3e}")
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(s)) and st[0] == cmin == c.min(), name
    assert np.array_equal(p.mean(), a), name
    assert err <= lim, f"{name}: off by {err:.3e} > {lim:.3e} ({errs})"
    return a


def dense_case(table, model, T, N):
    """Two consecutive solves from a warm start off zero at lambda = the standard deviation of a scout's costs."""
    mode = fc.fused_mode(N)
    kw = dict(mode=mode, row=T * fc.DIM_CONTROL[model])
    expl = fc.EXPLORATION if fc.split_inside_a_block(N, _cu()) else 0.0
    mean = (np.random.default_rng(T * 131 + N).standard_normal((T, fc.DIM_CONTROL[model])) * 0.2).astype(f32)
    scout = Raw(model, T, N, mode=0, exploration=expl)
    scout.set_mean(mean)
    lam = float(np.std(scout.rollout(1).astype(np.float64)))
    scout.close()
    if not lam > 0.0:   # (one sample)
        lam = 1.0
    p = Raw(model, T, N, mode=mode, exploration=expl)
    p.set_mean(mean)
    name = f"{model} T{T} N{N}" + (" explore" if expl else "")
    a = check_dense(table, name + " solve 1", p, 1, lam, mean, **kw)
    check_dense(table, name + " solve 2", p, 2, lam, a, **kw)
    p.close()


@pytest.mark.parametrize("N", fc.SIZE_NS)
def test_dense_weights_at_every_size(N):
    dense_case("sizes", "pendulum", fc.SIZE_T, N)


@pytest.mark.parametrize("model,T", fc.ROW_TABLE, ids=[f"{m}-T{T}" for m, T in fc.ROW_TABLE])
def test_dense_weights_at_every_row_shape(model, T):
    dense_case("rows", model, T, fc.ROW_TABLE_N)


def test_a_row_too_wide_takes_the_multi_kernel_path():
    model, T = fc.ROW_TOO_WIDE
    N = fc.ROW_TABLE_N
    assert fc.geometry(N, _cu(), row=T * fc.DIM_CONTROL[model]) is None
    p = Raw(model, T, N)
    p.set_mean(np.zeros(T))
    a, s, st, c = p.solve(1, 20.0)
    assert took(p.h) == (0, 0) and p.h.lib.mppi_fused_error(p.h.h) == 0
    assert np.all(np.isfinite(a)) and st[0] == c.min()
    p.close()


# ------------------------------------------------------------------------------ (d) searches
_SEARCHES = ([("ESSPS", N, N == 4096) for N in (1000, 4096, 4097, 16384)] + [("LBPS", N, False) for N in (1000, 4096, 4097, 16384)]
             + [("MPO", N, False) for N in (1000, 4096)])


@pytest.mark.parametrize("rule,N,sg", _SEARCHES, ids=[f"{r}-N{N}" + ("-sg" if sg else "") for r, N, sg in _SEARCHES])
def test_searches_find_the_multi_kernel_temperature(rule, N, sg):
    """Three closed-loop ticks of the default solver against a multi-kernel twin that is fed the same warm start."""
    T = 15
    kw = dict(use_sg_filter=True) if sg else {}
    if rule == "ESSPS":
        kw.update(essps_target_ess=N / 10.0, lambda_min=1e-3, lambda_max=1e5)
    if rule == "LBPS":
        kw.update(lbps_search="grid")
    fused, x0 = make("pendulum", T, N, rule, **kw)
    multi, _ = make("pendulum", T, N, rule, **kw)
    multi.set_option("fused_solve", 0)
    assert fused._one_call and multi._one_call
    geo = dict(search=rule != "MPO", mode=1, row=T)
    x = x0.cuda()
    for k in range(3):
        name = f"{rule} N{N} tick {k}"
        if k:
            multi.set_warm_start(fused._previous_action_seq.cpu().numpy(), fused._actions_history_for_sg if sg else None)
        a1, s1 = fused.forward(x)
        a2, s2 = multi.forward(x)
        G, spb = assert_single_launch(fused._h, N, name, **geo)
        assert took(multi._h) == (0, 0), name
        assert torch.equal(fused._costs, multi._costs) and fused.last_stats()["cmin"] == multi.last_stats()["cmin"], name
        l1, l2 = fused._last_lambda, multi._last_lambda
        costs = fused._costs.cpu().numpy()
        dl = abs(l1 - l2) / l2
        line = f"[fused] search {name} G{G} spb{spb}: lambda {l1:.9g} vs {l2:.9g} (rel {dl:.2e})"
        if rule == "ESSPS":
            ess = weights64(costs, l1)[1]
            print(line + f", float64 ESS {ess:.4f} for a target of {N / 10.0}")
            assert kw["lambda_min"] < l1 < kw["lambda_max"], name
            assert abs(ess - N / 10.0) <= 1e-4 * N / 10.0, f"{name}: ESS {ess} at the single launch's temperature"
        else:
            print(line)
        if rule == "LBPS":
            assert same_lbps_minimum(costs, l1, l2), (name, l1, l2)
        else:
            assert dl <= (3e-6 if rule == "ESSPS" and k else 1e-6), (name, l1, l2)
        assert rel_err(a1.cpu().numpy(), a2.cpu().numpy()) < 2e-6 + 20 * dl, name   # (the bound of the parity suite's twin test)
        x = s1[0, 1].clone()


# ------------------------------------------------------------------------------ (e) handover between the paths
@pytest.mark.parametrize("N", [1000, 6145])
def test_alternating_paths_hand_the_minimum_slot_over(N):
    """The single launch resets the OTHER minimum slot for the next multi-kernel rollout, which accumulates into it with
    atomicMin: a solver that alternates between the paths sees the costs and the minimum of one that never leaves the
    multi-kernel path."""
    T, lam = 15, 20.0
    both, x0 = make("pendulum", T, N, lam)
    multi, _ = make("pendulum", T, N, lam)
    multi.set_option("fused_solve", 0)
    x = x0.cuda()
    G, spb = fc.geometry(N, _cu(), mode=2, row=T)
    lim = fc.limit(G, spb, fc.row_shape(T, 1)[0], TOL)
    for k, mode in enumerate((2, 0, 2, 0)):
        name = f"N{N} tick {k} fused_solve {mode}"
        both.set_option("fused_solve", mode)
        if k:
            multi.set_warm_start(both._previous_action_seq.cpu().numpy())
        a1, s1 = both.forward(x)
        a2, s2 = multi.forward(x)
        if mode:
            assert_single_launch(both._h, N, name, mode=2, row=T)
        else:
            assert took(both._h) == (0, 0), name
        assert took(multi._h) == (0, 0), name
        costs = both._costs.cpu().numpy()
        assert np.array_equal(costs, multi._costs.cpu().numpy()), name
        assert both.last_stats()["cmin"] == multi.last_stats()["cmin"] == costs.min(), name
        U = both._perturbed_action_seqs.cpu().numpy().reshape(N, -1).astype(np.float64)
        w = weights64(costs, lam)[0]
        scale = (w @ np.abs(U)) / w.sum()
        err = float(np.max(np.abs(a1.cpu().numpy().ravel().astype(np.float64) - a2.cpu().numpy().ravel()) / scale))
        worst["handover"] = max(worst.get("handover", 0.0), err)
        print(f"[fused] handover {name}: action vs the multi-kernel twin {err:.3e} (limit {lim:.3e}); max so far {worst['handover']:.3e}")
        assert err <= lim, f"{name}: {err:.3e} > {lim:.3e}"
        x = s1[0, 1].clone()
