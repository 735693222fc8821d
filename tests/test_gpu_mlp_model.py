"""The learned-dynamics models (MPPI_MODEL_MLP41 / MLP42: envs/mlp_model.py, mppi_set_mlp) on a real MI355X.

Costs and clamped actions come from the C ABI's individual entry points (test_gpu_action_cost.Rig); the references are the
two evaluations of tests/mlp_ref.py on the EXPORTED actions.

  relu, math 0   every sample's cost equals the fp32 restatement bit for bit — by the rollout kernel with regenerated noise
                 and with tiles, by the single launch, with fused_solve = 0 — and so do the states of get_top_samples(8).
  tanh / math 1  costs against the float64 evaluation.  The limit is not fixed in advance: per case, 4 x the distance of the
                 numpy fp32 restatement from float64 on the same actions (the reference's own rounding band), floored at
                 2 * 2^-24 * sum |terms of the cost| (mlp_ref.band).  The measured ratio is printed as an `[mlp]` line.
  mapping = 1    (the comparison kernel: a wavefront per trajectory) adds the T + 1 stage costs with a wave reduction in fp32,
                 not in the order the restatement fixes, for every model; it is held to the float64 band at every level.
Shapes: N in {64, 100, 4160} (one tile, a ragged tile, 65 tiles), T in {1, 4, 5, 8, 9} for mlp41 (four steps per float4
group) and {1, 2, 3, 7, 8} for mlp42: the smallest that reach every copy of the horizon loop.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import action_cost_ref as acref
import mlp_ref as R
from helpers import rel_err
from test_gpu_action_cost import Rig, term
from test_gpu_covariance import _need_gpu, weights64
from test_gpu_fused_geometry import took

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
worst = {"ratio": 0.0}


def build(cs, T, N, lam=1.0, tag=True, **kw):
    """(solver, model) around a case of the table; tag=False hides the native tags behind plain lambdas (generic path)."""
    _need_gpu()
    from envs import MLPModel
    from pi_mpc.mppi import MPPI

    P = cs["params"]
    model = MLPModel(cs["Ws"], cs["bs"], activation=cs["activation"], residual=cs["residual"], goal=P[:4], q=P[4:8], r=P[8:])
    assert np.array_equal(model.table, cs["table"])
    dyn, cost = (model.dynamics, model.cost) if tag else ((lambda s, a: model.dynamics(s, a)), (lambda s, a, i: model.cost(s, a, i)))
    solver = MPPI(horizon=T, num_samples=N, dim_state=4, dim_control=cs["dc"], dynamics=dyn, cost_func=cost,
                  u_min=torch.tensor(cs["u_min"]), u_max=torch.tensor(cs["u_max"]), sigmas=torch.tensor(cs["sigmas"]),
                  lambda_=lam, **kw)
    assert (solver._model == model.model_name) if tag else (solver._model is None)
    return solver, model


class MlpRig(Rig):
    def __init__(self, cs, T, N, math=0, mode=None, **kw):
        self.cs = cs
        solver, self.mlp = build(cs, T, N, **kw)
        super().__init__(self.mlp.model_name, T, N, solver=(solver, torch.from_numpy(R.X0.copy())))
        self.h.call("mppi_set_option", b"math", math)
        if mode is not None:
            self.h.call("mppi_set_option", b"fused_solve", mode)
        rng = np.random.default_rng(T * 1000 + N)
        self.mean0 = rng.uniform(f32(cs["u_min"]), f32(cs["u_max"]), (T, cs["dc"])).astype(f32)
        self.set_mean(self.mean0)

    def ref(self, U, dtype=f32, table=None):
        cs = self.cs
        return R.rollout(cs["table"] if table is None else table, cs["params"], cs["hidden_layers"], cs["activation"],
                         cs["residual"], R.X0, U, dtype)

    def top_states(self, k, lam):
        st, w = torch.empty(k, self.T + 1, 4, device="cuda"), torch.empty(k, device="cuda")
        self.h.call("mppi_top_samples", k, float(lam), st.data_ptr(), w.data_ptr(), self.solver._stream())
        torch.cuda.synchronize()
        return st.cpu().numpy(), w.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(name, got, want):
    bad = int(np.sum(bits(got) != bits(want)))
    assert bad == 0, f"{name}: {bad} of {got.size} values differ from the fp32 restatement"


def check_top_states(name, rig, c, S32, lam, k=8):
    st, w = rig.top_states(k, lam)
    assert np.all(np.diff(w) <= 0), name
    order = np.argsort(c, kind="stable")
    kth = c[order[k - 1]]
    if len(np.unique(c[order[:k + 1]])) == min(k + 1, len(c)):  # no ties around the cut: the order is determined
        same_bits(f"{name}: top states", st, S32[order[:k]])
    else:
        cand = S32[c <= kth]
        for row in st:
            assert any(np.array_equal(bits(row), bits(x)) for x in cand), name


def in_band(name, rig, c, U):
    c32, _, mag = rig.ref(U)
    c64, _, _ = rig.ref(U, f64)
    limit, yard = R.band(c32, c64, mag)
    err = np.abs(c.astype(f64) - c64)
    ratio = float(err.max() / yard) if yard > 0 else 0.0
    worst["ratio"] = max(worst["ratio"], ratio)
    print(f"[mlp] {name}: ratio {ratio:.2f} of the fp32 band {yard:.3g}; max err {err.max():.3g}, largest so far {worst['ratio']:.2f}")
    assert np.all(np.isfinite(c)), name
    over = err > limit
    assert not over.any(), f"{name}: {int(over.sum())} costs beyond the band, worst {err.max():.3g} against {limit[np.argmax(err - limit)]:.3g}"


RELU = [c[0] for c in R.CASES if c[3] == "relu"]
ALL = [c[0] for c in R.CASES]
LAM = 2.0


# ------------------------------------------------------------------------------ 1. relu, math 0: bit for bit
@pytest.mark.parametrize("name", RELU)
def test_relu_math0_costs_and_top_states_bit_for_bit(name):
    cs = R.case(name)
    for T in R.HORIZONS[cs["dc"]]:
        for N in R.SAMPLES:
            rig = MlpRig(cs, T, N)
            tagname = f"{name} T{T} N{N}"
            c = rig.rollout(3)                       # the rollout kernel, noise regenerated in registers
            U = rig.actions_around(rig.mean0)
            c32, S32, _ = rig.ref(U)
            same_bits(f"{tagname} regenerated", c, c32)
            rig.h.call("mppi_set_option", b"noise_regen", 0)
            same_bits(f"{tagname} tiles", rig.rollout(3), c32)
            rig.h.call("mppi_set_option", b"noise_regen", 1)
            _, _, _, cs_ = rig.solve(3, LAM)         # mppi_solve: the single launch up to 4096 samples
            assert (took(rig.h) != (0, 0)) == (N <= 4096), tagname
            same_bits(f"{tagname} mppi_solve", cs_, c32)
            check_top_states(tagname, rig, c32, S32, LAM)
            rig.close()


@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp42_relu_2l_abs", "mlp41_relu_1l_abs", "mlp42_relu_1l_res"])
def test_relu_math0_multi_kernel_solve(name):
    cs = R.case(name)
    for T in R.HORIZONS[cs["dc"]]:
        rig = MlpRig(cs, T, 100, mode=0)
        a, s, st, c = rig.solve(4, LAM)
        assert took(rig.h) == (0, 0)
        U = rig.actions_around(rig.mean0)
        c32, S32, _ = rig.ref(U)
        same_bits(f"{name} T{T} fused_solve=0", c, c32)
        check_top_states(f"{name} T{T}", rig, c32, S32, LAM)
        # the returned state sequence is the rollout of the returned actions (finalize_kernel's copy of the step)
        _, Sa, _ = rig.ref(a[None])
        same_bits(f"{name} T{T} state_seq", s, Sa[0])
        rig.close()


# ------------------------------------------------------------------------------ 2. tanh, and the fast level: the band
@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("name", ALL)
def test_costs_within_the_fp32_band_of_float64(name, math):
    cs = R.case(name)
    for T in R.HORIZONS[cs["dc"]]:
        for N in R.SAMPLES if T == R.HORIZONS[cs["dc"]][-1] else (64, 100):
            rig = MlpRig(cs, T, N, math=math)
            c = rig.rollout(5)
            U = rig.actions_around(rig.mean0)
            in_band(f"{name} math {math} T{T} N{N} rollout", rig, c, U)
            rig.h.call("mppi_set_option", b"noise_regen", 0)
            ct = rig.rollout(5)
            rig.h.call("mppi_set_option", b"noise_regen", 1)
            in_band(f"{name} math {math} T{T} N{N} tiles", rig, ct, U)
            if N <= 4096:
                _, _, _, c1 = rig.solve(5, LAM)
                assert took(rig.h) != (0, 0)
                in_band(f"{name} math {math} T{T} N{N} single launch", rig, c1, U)
                rig.set_mean(rig.mean0)              # (the solve stored its own warm start)
                rig.h.call("mppi_set_option", b"fused_solve", 0)
                _, _, _, c0 = rig.solve(5, LAM)
                assert took(rig.h) == (0, 0)
                in_band(f"{name} math {math} T{T} N{N} fused_solve=0", rig, c0, U)
            rig.close()


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp42_tanh_2l_abs"])
def test_wavefront_per_trajectory_mapping(name, math):
    cs = R.case(name)
    T = R.HORIZONS[cs["dc"]][-1]
    rig = MlpRig(cs, T, 100, math=math)
    rig.h.call("mppi_set_option", b"mapping", 1)
    c = rig.rollout(6)
    in_band(f"{name} math {math} mapping 1", rig, c, rig.actions_around(rig.mean0))
    rig.close()


# ------------------------------------------------------------------------------ 3. forward() end to end
def sg64(a, coeffs):
    """The Savitzky-Golay step of the first solve (zero history) in float64: [zeros(T-1); a], flip-padded, keep the last T."""
    T, dc = a.shape
    pad = len(coeffs) // 2
    y = np.concatenate([np.zeros((T - 1, dc)), a.astype(f64)])
    yp = np.concatenate([y[:pad][::-1], y, y[-pad:][::-1]])
    out = sum(yp[j:j + len(y)] * f64(cj) for j, cj in enumerate(coeffs))
    return out[-T:]


def check_forward(name, solver, cs, a, s, lam, table=None):
    c = solver._costs.cpu().numpy()
    U = solver._perturbed_action_seqs.cpu().numpy()
    e, _ = weights64(c, lam)
    a64 = np.tensordot(e, U.astype(f64), axes=1) / e.sum()
    if solver._use_sg_filter:
        a64 = sg64(a64, solver._coeffs)
    a, s = a.cpu().numpy(), s.cpu().numpy()[0]
    assert np.max(np.abs(a - a64)) <= 1e-5, f"{name}: action_seq {np.max(np.abs(a - a64)):.3g} from the float64 softmax"
    _, S64, _ = R.rollout(cs["table"] if table is None else table, cs["params"], cs["hidden_layers"], cs["activation"],
                          cs["residual"], R.X0, a[None], f64)
    assert np.max(np.abs(s - S64[0])) <= 1e-5, f"{name}: state_seq {np.max(np.abs(s - S64[0])):.3g} from the float64 rollout"
    return c, U


FORWARD = [("fixed", dict(lam=2.0)), ("essps", dict(lam="ESSPS", essps_target_ess=60.0, lambda_min=0.01, lambda_max=100.0)),
           ("sg", dict(lam=2.0, use_sg_filter=True))]


@pytest.mark.parametrize("rule,kw", FORWARD)
@pytest.mark.parametrize("name,T,N", [("mlp41_tanh_2l_res", 9, 1000), ("mlp42_tanh_2l_abs", 7, 4160), ("mlp42_relu_1l_res", 8, 600)])
def test_forward_end_to_end(name, T, N, rule, kw):
    cs = R.case(name)
    solver, _ = build(cs, T, N, **kw)
    a, s = solver.forward(torch.from_numpy(R.X0.copy()).cuda())
    lam = solver._last_lambda if rule == "essps" else kw["lam"]
    check_forward(f"{name} {rule}", solver, cs, a, s, lam)


# ------------------------------------------------------------------------------ 4. against the generic path
@pytest.mark.parametrize("name,T,N", [("mlp41_tanh_2l_res", 9, 600), ("mlp42_tanh_2l_abs", 7, 600)])
def test_same_controller_without_the_tag(name, T, N):
    """The same plugin behind plain lambdas (the solver's generic path evaluates the torch callables), the same injected noise,
    lambda with |c| / lambda <= 10.  The costs of both paths lie within the tanh band of the float64 evaluation, and the two
    action sequences agree within the same band taken for the action sequence: 4 x the distance between the float64 softmax
    average over the fp32 restatement's costs and the one over the float64 costs, floored at 2 * 2^-24 * sum w |U|."""
    cs = R.case(name)
    x0 = torch.from_numpy(R.X0.copy()).cuda()
    rng = np.random.default_rng(9)
    eps = torch.from_numpy((rng.standard_normal((N, T, cs["dc"])) * f32(cs["sigmas"])).astype(f32))
    U0 = np.clip(eps.numpy(), f32(cs["u_min"]), f32(cs["u_max"]))  # (first solve: zero warm start)
    ref = lambda dtype: R.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], R.X0, U0, dtype)  # noqa: E731
    (c32, _, mag), (c64, _, _) = ref(f32), ref(f64)
    lam = float(np.abs(c64).max()) / 10.0
    outs = []
    for tag in (True, False):
        solver, _ = build(cs, T, N, lam=lam, tag=tag)
        solver.inject_noise(eps)
        a, s = solver.forward(x0)
        outs.append((a.cpu().numpy(), solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy()))
    (an, cn, Un), (ag, cg, Ug) = outs
    assert np.array_equal(Un, U0) and np.array_equal(Ug, U0)
    assert np.max(np.abs(cn)) / lam <= 10.0 * (1 + 1e-5)
    limit, yard = R.band(c32, c64, mag)
    for label, c in (("native", cn), ("generic", cg)):
        err = np.abs(c.astype(f64) - c64)
        print(f"[mlp] {name} {label} path costs: ratio {err.max() / yard:.2f} of the fp32 band {yard:.3g}")
        assert np.all(err <= limit), f"{name} {label}: {err.max():.3g}"

    def avg(c):
        e = np.exp(-(c.astype(f64) - c.astype(f64).min()) / lam)
        w = e / e.sum()
        return np.tensordot(w, U0.astype(f64), axes=1), np.tensordot(w, np.abs(U0).astype(f64), axes=1)

    (a32, _), (a64, wabs) = avg(c32), avg(c64)
    yard_a = float(np.max(np.abs(a32 - a64)))
    lim_a = np.maximum(4.0 * yard_a, 2.0 * 2.0 ** -24 * wabs)
    d = np.abs(an.astype(f64) - ag.astype(f64))
    print(f"[mlp] {name}: native against generic action_seq {d.max():.3g}, ratio {d.max() / max(yard_a, 1e-300):.2f} of the "
          f"fp32 band {yard_a:.3g}")
    assert np.all(d <= lim_a), f"{name}: action sequences differ by {d.max():.3g}, band {lim_a.min():.3g}"


# ------------------------------------------------------------------------------ 5. the table between solves, errors
def test_update_weights_between_two_solves():
    cs, cs2 = R.case("mlp41_relu_2l_res"), R.case("mlp41_relu_2l_abs")
    rig = MlpRig(cs, 9, 4160)
    c = rig.rollout(3)
    U = rig.actions_around(rig.mean0)
    same_bits("before", c, rig.ref(U)[0])
    Ws2 = [w.copy() for w in cs2["Ws"]]
    Ws2[-1] = (Ws2[-1] * f32(0.05)).astype(f32)  # (residual stays on: keep the step small)
    rig.mlp.update_weights(Ws2, cs2["bs"])
    assert rig.mlp.version == 1
    rig.solver._refresh_model_inputs()              # what every forward() does first
    c2 = rig.rollout(3)
    table2 = R.pack(Ws2, cs2["bs"], 1)
    same_bits("after update_weights", c2, rig.ref(U, table=table2)[0])
    assert not np.array_equal(c, c2)
    # ... and through forward(): two solves, new weights in between, each against its own table
    solver, model = build(cs, 9, 600, lam=2.0)
    x0 = torch.from_numpy(R.X0.copy()).cuda()
    solver.set_option("math", 0)
    a, s = solver.forward(x0)
    c1, U1 = solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy()
    same_bits("forward 1", c1, R.rollout(cs["table"], cs["params"], 2, "relu", True, R.X0, U1)[0])
    model.update_weights(Ws2, cs2["bs"])
    a, s = solver.forward(x0)
    c2, U2 = solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy()
    same_bits("forward 2", c2, R.rollout(table2, cs["params"], 2, "relu", True, R.X0, U2)[0])
    rig.close()


def test_missing_table_and_bad_tables_raise():
    _need_gpu()
    from mppi_playground_amd import _capi

    cs = R.case("mlp42_relu_2l_res")
    cfg = _capi.MppiConfig()
    cfg.model, cfg.horizon, cfg.dim_state, cfg.dim_control = _capi.MODEL_IDS["mlp42"], 7, 4, 2
    cfg.num_samples, cfg.sample_offset, cfg.inherit_count = 100, 0, 100
    for k in range(2):
        cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = cs["u_min"][k], cs["u_max"][k], cs["sigmas"][k]
    cfg.seed, cfg.device = 1, 0
    h = _capi.Handle(cfg)
    par = np.ascontiguousarray(cs["params"], f32)
    h.call("mppi_set_model_params", par.ctypes.data_as(C.c_void_p), 10)
    x0 = torch.from_numpy(R.X0.copy()).cuda()
    h.call("mppi_set_state", x0.data_ptr(), 1, None)
    h.call("mppi_sample", 1, None)
    with pytest.raises(_capi.MppiError, match=r"\(-3\).*weight table"):  # MPPI_E_STATE
        h.call("mppi_rollout_cost", None)
    with pytest.raises(_capi.MppiError, match=r"\(-3\)"):
        h.call("mppi_solve", None, 1, 1.0, None, None, None, None)
    tab = np.ascontiguousarray(cs["table"], f32)
    put = lambda t, n, hl=2, act=0, res=1: h.call("mppi_set_mlp", t.ctypes.data_as(C.c_void_p), n, hl, act, res, None)  # noqa: E731
    for n in (tab.size - 1, R.n_floats(1), 0):       # wrong counts (mlp41's among them)
        with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
            put(tab, n)
    for bad in (np.nan, np.inf, -np.inf):
        t = tab.copy()
        t[700] = bad
        with pytest.raises(_capi.MppiError, match=r"\(-1\).*finite"):
            put(t, t.size)
    for kw in (dict(hl=0), dict(hl=3), dict(act=2), dict(res=2)):
        with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
            put(tab, tab.size, **kw)
    with pytest.raises(_capi.MppiError, match=r"\(-1\)"):  # wrong parameter count
        h.call("mppi_set_model_params", par.ctypes.data_as(C.c_void_p), 9)
    put(tab, tab.size)
    h.call("mppi_rollout_cost", None)                # now it runs
    c = torch.empty(100, device="cuda")
    h.call("mppi_get_costs", c.data_ptr(), 1, None)
    torch.cuda.synchronize()
    assert torch.isfinite(c).all()
    # a handle of another model refuses the table; mppi_model_step refuses these ids
    from test_gpu_covariance import make

    pend, _ = make("pendulum", 8, 64, 1.0)
    with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
        pend._h.call("mppi_set_mlp", tab.ctypes.data_as(C.c_void_p), tab.size, 2, 0, 1, None)
    s, a = torch.zeros(4, device="cuda"), torch.zeros(2, device="cuda")
    rc = h.lib.mppi_model_step(_capi.MODEL_IDS["mlp42"], par.ctypes.data_as(C.c_void_p), 10, None, None, s.data_ptr(),
                               a.data_ptr(), s.data_ptr(), None, 0.0, None, None)
    assert rc == -1
    h.close()
    # the Python helper refuses wrong dims before anything reaches the device
    from envs import MLPModel

    with pytest.raises(ValueError):
        MLPModel([np.zeros((8, 7)), np.zeros((4, 8))], [np.zeros(8), np.zeros(4)])
    with pytest.raises(ValueError):
        MLPModel([np.full((8, 5), np.inf), np.zeros((4, 8))], [np.zeros(8), np.zeros(4)])
    with pytest.raises(AssertionError):              # a 2-control model on a 1-control solver
        solver, _ = build(dict(cs, dc=1, u_min=[-1.0], u_max=[1.0], sigmas=[1.0]), 7, 64)


def test_callables_of_two_models_do_not_run_as_one():
    """dynamics of one MLPModel with the cost of another: the device would take table and parameters from the cost's owner
    alone, so the pair is not a native model — it runs on the generic path, each callable with its own owner's data."""
    _need_gpu()
    from envs import MLPModel
    from pi_mpc.mppi import MPPI

    a, b = R.case("mlp41_tanh_2l_res"), R.case("mlp41_tanh_2l_abs")
    ma = MLPModel(a["Ws"], a["bs"], activation="tanh", residual=True)
    mb = MLPModel(b["Ws"], b["bs"], activation="tanh", residual=False)
    kw = dict(horizon=5, num_samples=64, dim_state=4, dim_control=1, u_min=torch.tensor(a["u_min"]),
              u_max=torch.tensor(a["u_max"]), sigmas=torch.tensor(a["sigmas"]), lambda_=1.0)
    assert MPPI(dynamics=ma.dynamics, cost_func=mb.cost, **kw)._model is None
    assert MPPI(dynamics=ma.dynamics, cost_func=ma.cost, **kw)._model == "mlp41"


# ------------------------------------------------------------------------------ 6. the opt-ins
@pytest.mark.parametrize("name,T", [("mlp41_relu_2l_res", 9), ("mlp42_relu_2l_abs", 7), ("mlp41_tanh_2l_res", 8)])
def test_action_cost_term(name, T):
    """costs == fl32(c0 + fl32(kappa * A)) with c0 the same handle's rollout at weight 0 (tests/action_cost_ref.py)."""
    cs = R.case(name)
    for N in (100, 4160):
        rig = MlpRig(cs, T, N, action_cost=True)
        term(rig, 0.0, 3.0)
        c0 = rig.rollout(3)
        term(rig, 1.0, 3.0)
        c1 = rig.rollout(3)
        U = rig.actions_around(rig.mean0)
        g = acref.g32(rig.mean0, f32(cs["sigmas"]))
        acref.check(f"{name} N{N}", c1, c0, acref.kappa32(1.0, 3.0), g, U)
        if cs["activation"] == "relu":  # c0 itself is the restatement's
            same_bits(f"{name} N{N} c0", c0, rig.ref(U)[0])
        assert np.any(c1 != c0)
        rig.close()


@pytest.mark.parametrize("kw", [dict(noise_beta=0.9), dict(adapt_covariance=True)], ids=["noise_beta", "adapt_covariance"])
@pytest.mark.parametrize("name,T", [("mlp41_tanh_2l_res", 9), ("mlp42_tanh_2l_abs", 7)])
def test_colored_noise_and_covariance_adaptation_solve(name, T, kw):
    cs = R.case(name)
    solver, _ = build(cs, T, 1000, lam=2.0, **kw)
    x0 = torch.from_numpy(R.X0.copy()).cuda()
    for tick in range(2):  # (the second solve draws from the adapted table / around a non-zero mean)
        a, s = solver.forward(x0)
        check_forward(f"{name} {list(kw)[0]} tick {tick}", solver, cs, a, s, 2.0)


def test_deep_copy_continues_bit_identically():
    cs = R.case("mlp42_tanh_2l_abs")
    solver, model = build(cs, 7, 1000, lam=2.0)
    x0 = torch.from_numpy(R.X0.copy()).cuda()
    solver.forward(x0)
    twin = copy.deepcopy(solver)
    assert twin._cost_owner is not model and twin._model == "mlp42"
    for tick in range(3):
        a, s = solver.forward(x0)
        b, r = twin.forward(x0)
        assert torch.equal(a, b) and torch.equal(s, r) and torch.equal(solver._costs, twin._costs), tick
    sd = solver.state_dict()
    assert "_extra_state" in sd
    twin.load_state_dict(sd)


def _shard_worker(rank, world, port, q):
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["MPPI_EXCHANGE"] = "nccl"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import mppi_playground_amd  # noqa: F401

        cs = R.case("mlp41_tanh_2l_res")
        solver, _ = build(cs, 9, 1024, lam=2.0, shard_samples=True)
        a, s = solver.forward(torch.from_numpy(R.X0.copy()).cuda())
        q.put((rank, a.cpu().numpy(), s.cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_rank_sharded_solve_matches_the_unsharded_solve():
    """shard_samples=True with two ranks on this device (gloo), as tests/test_gpu_parity.py measures the shipped models: the
    first solve within 2e-6 (relative to the largest entry) of the unsharded one, the ranks equal to each other."""
    _need_gpu()
    import socket

    import torch.multiprocessing as mp

    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    cs = R.case("mlp41_tanh_2l_res")
    single, _ = build(cs, 9, 1024, lam=2.0)
    a, s = single.forward(torch.from_numpy(R.X0.copy()).cuda())
    for r in res:
        assert rel_err(r[1], a.cpu().numpy()) < 2e-6 and rel_err(r[2], s.cpu().numpy()) < 2e-6
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
