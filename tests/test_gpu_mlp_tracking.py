"""Tracking costs of the learned-dynamics models (per-step goals, wrapped angle errors: mppi_set_mlp_reference,
mppi_set_mlp_angular; envs.MLPModel.set_reference / angular=) on a real MI355X.

Costs and clamped actions come from the C ABI's individual entry points (test_gpu_action_cost.Rig); the reference is the numpy
restatement of tests/mlp_track_ref.py on the EXPORTED actions — the inputs tests/test_mlp_tracking_host.py has shown to wrap
(both signs of k) and to expose an off-by-one row.

  relu, math 0   every sample's cost equals the restatement bit for bit — the rollout kernel with regenerated noise and with
                 tiles, mppi_solve in the single launch (N <= 4096) and with fused_solve = 0 — and a table padded with three
                 rows of NaN gives the same bits.
  the band       mapping = 1 (a wavefront per trajectory: the step index differs per lane), tanh and math 1 against float64
                 inside mlp_ref.band (4 x the fp32 restatement's own distance from float64, floored at 2 * 2^-24 * sum |terms|).
                 The measured ratio is printed as a `[mlp-track]` line.
Shapes: N in {64, 100, 4160} (one tile, a ragged tile, 65 tiles), T from HORIZONS of the two case tables: the smallest that
reach every copy of the horizon loop.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import action_cost_ref as acref
import mlp_track_ref as TR
import solve_ref as sr
from helpers import rel_err
from test_gpu_action_cost import Rig, current_mean, term
from test_gpu_covariance import _need_gpu
from test_gpu_feature_pairs import TOL
from test_gpu_fused_geometry import took
from test_gpu_mlp_model import same_bits

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
worst = {"ratio": 0.0}
LAM = 2.0


def model_of(cs, angular=None, Ws=None, bs=None):
    from envs import MLPModel, MLPModel8

    P, ds, DS = cs["params"], cs["ds"], cs["DS"]
    cls = MLPModel if DS == 4 else MLPModel8
    return cls(cs["Ws"] if Ws is None else Ws, cs["bs"] if bs is None else bs, activation=cs["activation"],
               residual=cs["residual"], goal=P[:ds], q=P[DS:DS + ds], r=P[2 * DS:], angular=cs["angular"] if angular is None else angular)


def put_reference(model, cs, ref, device=None):
    ds, DS = cs["ds"], cs["DS"]
    g, q = torch.from_numpy(ref[:, :ds].copy()), torch.from_numpy(ref[:, DS:DS + ds].copy())
    model.set_reference(g if device is None else g.to(device), q if device is None else q.to(device))


def build(cs, T, N, ref=None, angular=None, lam=1.0, tag=True, model=None, **kw):
    """(solver, model) around a case; ref: the padded table (None: no reference); tag=False hides the native tags."""
    _need_gpu()
    from pi_mpc.mppi import MPPI

    model = model_of(cs, angular) if model is None else model
    if ref is not None:
        put_reference(model, cs, ref)
    dyn, cost = (model.dynamics, model.cost) if tag else ((lambda s, a: model.dynamics(s, a)), (lambda s, a, i: model.cost(s, a, i)))
    solver = MPPI(horizon=T, num_samples=N, dim_state=cs["DS"], dim_control=cs["dc"], dynamics=dyn, cost_func=cost,
                  u_min=torch.tensor(cs["u_min"]), u_max=torch.tensor(cs["u_max"]), sigmas=torch.tensor(cs["sigmas"]),
                  lambda_=lam, **kw)
    assert (solver._model == cs["model"]) if tag else (solver._model is None)
    return solver, model


def x0_of(cs):
    return torch.from_numpy(f32(cs["x0"]).copy())


class TrackRig(Rig):
    def __init__(self, cs, T, N, ref="default", angular=None, math=0, mode=None, **kw):
        self.cs = cs
        self.table = TR.reference(cs, T) if isinstance(ref, str) else ref
        self.angular = cs["angular"] if angular is None else angular
        solver, self.mlp = build(cs, T, N, ref=self.table, angular=self.angular, **kw)
        super().__init__(cs["model"], T, N, solver=(solver, x0_of(cs)))
        assert (self.ds, self.dc) == (cs["DS"], cs["dc"])
        self.h.call("mppi_set_option", b"math", math)
        if mode is not None:
            self.h.call("mppi_set_option", b"fused_solve", mode)
        rng = np.random.default_rng(T * 1000 + N)
        self.mean0 = rng.uniform(f32(cs["u_min"]), f32(cs["u_max"]), (T, cs["dc"])).astype(f32)
        self.set_mean(self.mean0)

    def ref(self, U, dtype=f32, table="own", x0=None, weights=None):
        return TR.rollout(self.cs, self.table if isinstance(table, str) else table, self.angular, U, dtype, x0=x0, table=weights)

    def new_reference(self, table, device=None):
        put_reference(self.mlp, self.cs, table, device)
        self.solver._refresh_model_inputs()  # what every forward() does first
        self.table = table

    def nan_padded_reference(self, extra=3):
        """The same T rows and `extra` rows of NaN behind them, resident on the device.  (set_reference and a host table of
        the C ABI refuse values that are not finite: the rows are written in place, as a caller rewrites a device table.)"""
        want = TR.reference(self.cs, self.T, extra=extra)
        assert np.array_equal(want[:self.T], self.table[:self.T], equal_nan=True)
        put_reference(self.mlp, self.cs, TR.reference(self.cs, self.T, finite_extra=extra), "cuda")
        self.mlp.reference[self.T:] = float("nan")
        self.mlp.reference_changed()
        self.solver._refresh_model_inputs()
        got = self.mlp.reference.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True) and np.isnan(got[self.T:]).all()


def in_band(name, rig, c, U, refs=None):
    if refs is None:
        c32, _, mag = rig.ref(U)
        refs = (c32, rig.ref(U, f64)[0], mag)
    c32, c64, mag = refs
    limit, yard = TR.band(c32, c64, mag)
    err = np.abs(c.astype(f64) - c64)
    ratio = float(err.max() / yard) if yard > 0 else 0.0
    worst["ratio"] = max(worst["ratio"], ratio)
    print(f"[mlp-track] {name}: ratio {ratio:.2f} of the fp32 band {yard:.3g}; max err {err.max():.3g}, largest so far {worst['ratio']:.2f}")
    assert np.all(np.isfinite(c)), name
    over = err > limit
    assert not over.any(), f"{name}: {int(over.sum())} costs beyond the band, worst {err.max():.3g} against {limit[np.argmax(err - limit)]:.3g}"
    return refs


# ------------------------------------------------------------------------------ 1. relu, math 0: bit for bit
@pytest.mark.parametrize("name", TR.RELU)
def test_relu_math0_costs_bit_for_bit(name):
    cs = TR.case(name)
    for T in cs["horizons"]:
        for N in TR.SAMPLES:
            rig = TrackRig(cs, T, N)
            tagname = f"{name} T{T} N{N}"
            c = rig.rollout(3)                       # the rollout kernel, noise regenerated in registers
            U = rig.actions_around(rig.mean0)
            c32, S32, _ = rig.ref(U)
            same_bits(f"{tagname} regenerated", c, c32)
            rig.h.call("mppi_set_option", b"noise_regen", 0)
            same_bits(f"{tagname} tiles", rig.rollout(3), c32)
            rig.h.call("mppi_set_option", b"noise_regen", 1)
            a, s, _, cs_ = rig.solve(3, LAM)         # mppi_solve: the single launch up to 4096 samples, with a reference set
            assert (took(rig.h) != (0, 0)) == (N <= 4096), tagname
            same_bits(f"{tagname} mppi_solve", cs_, c32)
            same_bits(f"{tagname} state_seq of mppi_solve", s[:, :cs["ds"]], rig.ref(a[None])[1][0])
            rig.set_mean(rig.mean0)                  # (the solve stored its own warm start)
            rig.h.call("mppi_set_option", b"fused_solve", 0)
            _, _, _, c0 = rig.solve(3, LAM)          # the multi-kernel sequence
            assert took(rig.h) == (0, 0), tagname
            same_bits(f"{tagname} fused_solve=0", c0, c32)
            # the table with three more rows of NaN: the same bits on every path (nobody reads past row T - 1)
            rig.nan_padded_reference()
            rig.set_mean(rig.mean0)
            same_bits(f"{tagname} NaN-padded, fused_solve=0", rig.solve(3, LAM)[3], c32)
            rig.set_mean(rig.mean0)                  # (the solve stored its own warm start)
            same_bits(f"{tagname} NaN-padded, regenerated", rig.rollout(3), c32)
            rig.h.call("mppi_set_option", b"noise_regen", 0)
            same_bits(f"{tagname} NaN-padded, tiles", rig.rollout(3), c32)
            rig.h.call("mppi_set_option", b"noise_regen", 1)
            rig.h.call("mppi_set_option", b"fused_solve", 1)
            rig.set_mean(rig.mean0)
            same_bits(f"{tagname} NaN-padded, mppi_solve", rig.solve(3, LAM)[3], c32)
            # (the plain cost of the same actions is another number: the reference and the wrap are in these costs)
            assert not np.array_equal(c32, TR.rollout(cs, None, (), U)[0])
            rig.close()


# ------------------------------------------------------------------------------ 2. the band: tanh, math 1, mapping 1
# (relu at math 0 is held bit for bit above)
@pytest.mark.parametrize("name,math", [(n, math) for n in TR.CASES for math in (0, 1) if "_tanh_" in n or math])
def test_costs_within_the_fp32_band_of_float64(name, math):
    cs = TR.case(name)
    for T in cs["horizons"]:
        for N in TR.SAMPLES if T == cs["horizons"][-1] else (64, 100):
            rig = TrackRig(cs, T, N, math=math)
            tagname = f"{name} math {math} T{T} N{N}"
            c = rig.rollout(5)
            U = rig.actions_around(rig.mean0)
            refs = in_band(f"{tagname} rollout", rig, c, U)
            rig.h.call("mppi_set_option", b"noise_regen", 0)
            ct = rig.rollout(5)
            rig.h.call("mppi_set_option", b"noise_regen", 1)
            in_band(f"{tagname} tiles", rig, ct, U, refs)
            if N <= 4096:
                c1 = rig.solve(5, LAM)[3]
                assert took(rig.h) != (0, 0)
                in_band(f"{tagname} single launch", rig, c1, U, refs)
                rig.set_mean(rig.mean0)
                rig.h.call("mppi_set_option", b"fused_solve", 0)
                c0 = rig.solve(5, LAM)[3]
                assert took(rig.h) == (0, 0)
                in_band(f"{tagname} fused_solve=0", rig, c0, U, refs)
            rig.close()


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp42_tanh_1l_abs", "mlp81_relu_2l_res_s6", "mlp82_tanh_2l_res",
                                  "mlp84_relu_1l_abs", "mlp84_tanh_2l_res"])
def test_wavefront_per_trajectory_mapping(name, math):
    """mapping = 1: lane t evaluates the stage cost of step t (lane T the terminal cost with row T - 1), so the row address
    differs per lane."""
    cs = TR.case(name)
    for T in cs["horizons"]:
        rig = TrackRig(cs, T, 100, math=math)
        rig.h.call("mppi_set_option", b"mapping", 1)
        c = rig.rollout(6)
        in_band(f"{name} math {math} T{T} mapping 1", rig, c, rig.actions_around(rig.mean0))
        rig.h.call("mppi_set_option", b"mapping", 0)
        if math == 0 and cs["activation"] == "relu":
            same_bits(f"{name} T{T} mapping 0 on the same noise", rig.rollout(6), rig.ref(rig.actions_around(rig.mean0))[0])
        rig.close()


# ------------------------------------------------------------------------------ 3. the control-cost instantiation
@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp42_relu_1l_abs", "mlp81_relu_2l_res", "mlp82_relu_2l_res", "mlp84_relu_1l_abs"])
def test_action_cost_rollout_carries_the_tracking_cost(name):
    """The control-cost instantiations, regenerated noise and tiles: the tracking cost (bit for bit at math 0 with weight 0) plus
    the term, against tests/action_cost_ref.py on top of the restatement; at math 1 the weight-0 cost within the band."""
    cs = TR.case(name)
    for T in cs["horizons"][-2:]:
        for N in (100, 4160):
            rig = TrackRig(cs, T, N, action_cost=True)
            tagname = f"{name} T{T} N{N} action_cost"
            g = acref.g32(rig.mean0, rig.solver._sigmas.cpu().numpy())
            rig.h.call("mppi_sample", 4, rig.solver._stream())
            U = rig.actions_around(rig.mean0)
            c32 = rig.ref(U)[0]
            for regen in (1, 0):
                rig.h.call("mppi_set_option", b"noise_regen", regen)
                term(rig, 0.0, LAM)
                same_bits(f"{tagname} regen {regen} weight 0", rig.rollout(4), c32)
                term(rig, 1.0, LAM)
                c1 = rig.rollout(4)
                acref.check(f"{tagname} regen {regen}", c1, c32, acref.kappa32(1.0, LAM), g, U)
                if T > 1:
                    assert np.any(c1 != c32)
            rig.h.call("mppi_set_option", b"noise_regen", 1)
            rig.h.call("mppi_set_option", b"math", 1)
            term(rig, 0.0, LAM)
            c0 = rig.rollout(4)
            in_band(f"{tagname} math 1 weight 0", rig, c0, U)
            term(rig, 1.0, LAM)
            acref.check(f"{tagname} math 1", rig.rollout(4), c0, acref.kappa32(1.0, LAM), g, U)
            rig.close()


# ------------------------------------------------------------------------------ 4. particles and ensembles
def plain_costs(cs, model, x, T, N, ref):
    """The first solve of a fresh plain solver around `model` (its own table, the shared reference) from x, math 0 -> costs"""
    model = copy.deepcopy(model)
    solver, _ = build(cs, T, N, ref=ref, lam=LAM, model=model)
    solver.set_option("math", 0)
    solver.forward(torch.from_numpy(np.ascontiguousarray(x, f32)).cuda())
    return solver._costs.cpu().numpy()


@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp42_tanh_2l_res", "mlp82_relu_2l_res", "mlp84_tanh_1l_abs"])
def test_particles_through_members_equal_plain_handles(name):
    """P = 2 state particles through E = 2 members with a reference and the angular components: row m of particle_costs is what
    a plain handle holding member m's table computes from particles[m] with the same reference, bit for bit at math 0."""
    from envs import MLPEnsemble

    cs = TR.case(name)
    R = TR.module_of(name)
    parts = np.stack([f32(cs["x0"]), f32(cs["x0"]) + f32(0.1) * f32(np.resize([1.0, -0.5, 0.25, 0.3], cs["DS"]))]).astype(f32)
    parts[:, cs["ds"]:] = 0
    kw = dict(ds=cs["ds"]) if cs["DS"] == 8 else {}
    nets = [R.make_net(500 + e, cs["dc"], cs["hidden_layers"], cs["activation"], cs["residual"], **kw) for e in range(2)]
    for T in (3, cs["horizons"][-1]):
        ref = TR.reference(cs, T)
        for N in (64, 100):
            members = [model_of(cs, Ws=Ws, bs=bs) for Ws, bs in nets]
            ens = MLPEnsemble(members, nominal=0)
            es, _ = build(cs, T, N, ref=ref, lam=LAM, model=ens, risk="mean")
            assert all(torch.equal(m.reference, members[0].reference) for m in members)
            es.set_option("math", 0)
            es.set_state_particles(torch.from_numpy(parts), members=[1, 0])
            es.forward(x0_of(cs).cuda())
            E = es.particle_costs.cpu().numpy()
            assert E.shape == (2, N) and np.all(np.isfinite(E))
            for m, e in enumerate((1, 0)):
                same_bits(f"{name} T{T} N{N}: member {e} from particle {m}", E[m], plain_costs(cs, members[e], parts[m], T, N, ref))
                if cs["activation"] == "relu":  # (and the restatement with that member's weights)
                    U = es._perturbed_action_seqs.cpu().numpy()
                    same_bits(f"{name} T{T} N{N}: member {e} against the restatement", E[m],
                              TR.rollout(cs, ref, cs["angular"], U, x0=parts[m], table=members[e].table)[0])
            assert not np.array_equal(E[0], E[1])


# ------------------------------------------------------------------------------ 5. the hand-over
def _raw_handle(cs, T, N):
    from mppi_playground_amd import _capi

    cfg = _capi.MppiConfig()
    cfg.model, cfg.horizon, cfg.dim_state, cfg.dim_control = _capi.MODEL_IDS[cs["model"]], T, cs["DS"], cs["dc"]
    cfg.num_samples, cfg.sample_offset, cfg.inherit_count = N, 0, N
    for k in range(cs["dc"]):
        cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = cs["u_min"][k], cs["u_max"][k], cs["sigmas"][k]
    cfg.seed, cfg.device = 1, 0
    return _capi.Handle(cfg)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_device_table_rewritten_in_place_and_read_back():
    cs = TR.case("mlp82_relu_2l_res")
    T, N = 7, 100
    first, second = TR.reference(cs, T, seed=1), TR.reference(cs, T)
    rig = TrackRig(cs, T, N, ref=first)
    rig.new_reference(first, device="cuda")          # a device-resident table: copied in stream order, never meets the host
    held = rig.mlp.reference
    assert held.is_cuda
    c = rig.rollout(3)
    U = rig.actions_around(rig.mean0)
    same_bits("device table", c, rig.ref(U, table=first)[0])
    held.copy_(torch.from_numpy(second).cuda())      # rewritten in place on the device; the version is bumped
    rig.mlp.reference_changed()
    assert rig.mlp.reference is held
    rig.solver._refresh_model_inputs()
    c2 = rig.rollout(3)
    same_bits("rewritten in place", c2, rig.ref(U, table=second)[0])
    assert not np.array_equal(c, c2)
    # mppi_get_mlp_reference / mppi_get_mlp_angular return what was set
    n, mask = C.c_int(-1), C.c_uint32(99)
    rig.h.call("mppi_get_mlp_reference", None, C.byref(n), 0, None)
    rig.h.call("mppi_get_mlp_angular", C.byref(mask))
    assert n.value == T and mask.value == TR.mask(cs["angular"])
    host = np.full((T, 16), -1.0, f32)
    rig.h.call("mppi_get_mlp_reference", _vp(host), C.byref(n), 0, rig.solver._stream())
    dev = torch.full((T, 16), -1.0, device="cuda")
    rig.h.call("mppi_get_mlp_reference", dev.data_ptr(), None, 1, rig.solver._stream())
    torch.cuda.synchronize()
    same_bits("read back to the host", host, second)
    same_bits("read back on the device", dev.cpu().numpy(), second)
    # off again: the plain cost, and zero rows
    rig.mlp.set_reference(None)
    rig.solver._refresh_model_inputs()
    rig.h.call("mppi_get_mlp_reference", None, C.byref(n), 0, None)
    assert n.value == 0
    same_bits("reference off", rig.rollout(3), TR.rollout(cs, None, cs["angular"], U)[0])
    rig.close()


def test_clone_state_carries_table_and_mask():
    cs = TR.case("mlp41_relu_2l_res")
    T, N = 5, 100
    ref = TR.reference(cs, T)
    src, dst = _raw_handle(cs, T, N), _raw_handle(cs, T, N)
    par, tab = np.ascontiguousarray(cs["params"], f32), np.ascontiguousarray(cs["table"], f32)
    x0 = x0_of(cs).cuda()
    # the mask BEFORE the weights, the reference before both: the flags word has one owner
    src.call("mppi_set_mlp_reference", _vp(ref), T, 0, None)
    src.call("mppi_set_mlp_angular", TR.mask(cs["angular"]))
    src.call("mppi_set_model_params", _vp(par), int(par.size))
    src.call("mppi_set_mlp", _vp(tab), int(tab.size), cs["hidden_layers"], 0, int(cs["residual"]), None)
    for h in (src, dst):
        h.call("mppi_set_option", b"math", 0)
    src.call("mppi_set_state", x0.data_ptr(), 1, None)
    src.call("mppi_sample", 2, None)
    src.call("mppi_rollout_cost", None)
    dst.call("mppi_clone_state", src.h)
    n, mask = C.c_int(-1), C.c_uint32(0)
    dst.call("mppi_get_mlp_reference", None, C.byref(n), 0, None)
    dst.call("mppi_get_mlp_angular", C.byref(mask))
    assert n.value == T and mask.value == TR.mask(cs["angular"])
    back = np.zeros((T, 8), f32)
    dst.call("mppi_get_mlp_reference", _vp(back), None, 0, None)
    same_bits("the clone's table", back, ref)
    costs = []
    for h in (src, dst):
        h.call("mppi_sample", 2, None)
        h.call("mppi_rollout_cost", None)
        c = torch.empty(N, device="cuda")
        h.call("mppi_get_costs", c.data_ptr(), 1, None)
        torch.cuda.synchronize()
        costs.append(c.cpu().numpy())
    U = torch.empty(N, T, cs["dc"], device="cuda")
    dst.call("mppi_export_noise", None, U.data_ptr(), None)
    torch.cuda.synchronize()
    same_bits("the clone's costs", costs[1], costs[0])
    same_bits("against the restatement", costs[1], TR.rollout(cs, ref, cs["angular"], U.cpu().numpy())[0])
    src.close()
    dst.close()


def test_short_table_and_what_the_c_abi_refuses():
    from mppi_playground_amd import _capi
    from test_gpu_covariance import make

    cs = TR.case("mlp81_relu_2l_res")
    T, N = 5, 64
    h = _raw_handle(cs, T, N)
    par, tab = np.ascontiguousarray(cs["params"], f32), np.ascontiguousarray(cs["table"], f32)
    h.call("mppi_set_model_params", _vp(par), int(par.size))
    h.call("mppi_set_mlp", _vp(tab), int(tab.size), cs["hidden_layers"], 0, int(cs["residual"]), None)
    x0 = x0_of(cs).cuda()
    h.call("mppi_set_state", x0.data_ptr(), 1, None)
    ref = TR.reference(cs, T)
    h.call("mppi_set_mlp_reference", _vp(ref), T, 0, None)
    action, state, stats = (torch.full(s, 7.0, device="cuda") for s in ((T, 1), (1, T + 1, 8), (4,)))
    h.call("mppi_solve", None, 1, LAM, action.data_ptr(), state.data_ptr(), stats.data_ptr(), None)
    torch.cuda.synchronize()
    before = torch.empty(N, device="cuda")
    h.call("mppi_get_costs", before.data_ptr(), 1, None)
    kept = [t.clone() for t in (action, state, stats)]
    # rows < T: the solve fails with MPPI_E_STATE before anything is launched and no output buffer changes
    h.call("mppi_set_mlp_reference", _vp(ref), T - 1, 0, None)
    for entry in (lambda: h.call("mppi_solve", None, 2, LAM, action.data_ptr(), state.data_ptr(), stats.data_ptr(), None),
                  lambda: h.call("mppi_rollout_cost", None)):
        with pytest.raises(_capi.MppiError, match=r"\(-3\).*fewer rows than the horizon"):
            entry()
    torch.cuda.synchronize()
    after = torch.empty(N, device="cuda")
    h.call("mppi_get_costs", after.data_ptr(), 1, None)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(kept, (action, state, stats))) and torch.equal(before, after)
    h.call("mppi_set_mlp_reference", _vp(ref), T, 0, None)   # long enough again: it runs
    h.call("mppi_rollout_cost", None)
    # what the entry points refuse
    bad = ref.copy()
    for v in (np.nan, np.inf):
        bad[2, 9] = v
        with pytest.raises(_capi.MppiError, match=r"\(-1\).*finite"):
            h.call("mppi_set_mlp_reference", _vp(bad), T, 0, None)
    with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
        h.call("mppi_set_mlp_reference", _vp(ref), -1, 0, None)
    for mask in (1 << 8, 1 << 9, 0x1ff):
        with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
            h.call("mppi_set_mlp_angular", mask)
    h4 = _raw_handle(TR.case("mlp42_relu_2l_res"), T, N)
    with pytest.raises(_capi.MppiError, match=r"\(-1\)"):     # bit 4 on a 4-state handle
        h4.call("mppi_set_mlp_angular", 1 << 4)
    h4.call("mppi_set_mlp_angular", 0xF)
    cells = np.zeros((4, 4), np.uint8)  # a learned-dynamics handle has no maps: its map slot carries the reference
    with pytest.raises(_capi.MppiError, match=r"\(-1\).*no maps"):
        h4.call("mppi_upload_map", 0, _vp(cells), 4, 4, 1.0, 0.0, 0.0)
    h4.close()
    h.close()
    pend, _ = make("pendulum", 8, 64, 1.0)
    n = C.c_int(0)
    for call in (lambda: pend._h.call("mppi_set_mlp_reference", _vp(ref), T, 0, None),
                 lambda: pend._h.call("mppi_get_mlp_reference", None, C.byref(n), 0, None),
                 lambda: pend._h.call("mppi_set_mlp_angular", 1), lambda: pend._h.call("mppi_get_mlp_angular", None)):
        with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
            call()
    # the solver refuses a table shorter than its horizon before the solve
    solver, model = build(cs, T, N, ref=ref)
    solver.forward(x0)
    put_reference(model, cs, ref[:T - 1])
    with pytest.raises(ValueError, match="rows for a horizon"):
        solver.forward(x0)


# ------------------------------------------------------------------------------ 6. against the generic path
def _both_paths(cs, T, N, lam, math, ref):
    x0 = x0_of(cs).cuda()
    rng = np.random.default_rng(9 + T)
    eps = torch.from_numpy((rng.standard_normal((N, T, cs["dc"])) * f32(cs["sigmas"])).astype(f32))
    outs = []
    for tag in (True, False):
        solver, model = build(cs, T, N, ref=ref, lam=lam, tag=tag)
        if tag:
            solver.set_option("math", math)
        solver.inject_noise(eps)
        solver.forward(x0)
        outs.append((solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy(),
                     solver._state_seq_batch.cpu().numpy(), model))
    U0 = np.clip(eps.numpy(), f32(cs["u_min"]), f32(cs["u_max"]))  # (first solve: zero warm start)
    assert np.array_equal(outs[0][1], U0) and np.array_equal(outs[1][1], U0)
    return outs, U0


@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp42_relu_1l_abs", "mlp81_relu_2l_res_s6", "mlp84_relu_2l_res"])
def test_generic_path_means_the_same(name):
    """The same callables behind untagged lambdas (test_gpu_mlp8_model.py says where the two paths' totals are comparable bit
    for bit): every state of every sample, the totals at T = 1, the totals at a longer horizon within the band."""
    cs = TR.case(name)
    N = 100
    ref1 = TR.reference(cs, 1)
    ((cn, _, Sn, _), (cg, _, Sg, _)), U0 = _both_paths(cs, 1, N, 2.0, 0, ref1)
    same_bits(f"{name} T1: generic costs against fused", cg, cn)
    same_bits(f"{name} T1: generic states against fused", Sg, Sn)
    same_bits(f"{name} T1: fused against the restatement", cn, TR.rollout(cs, ref1, cs["angular"], U0)[0])
    T = cs["horizons"][-1]
    ref = TR.reference(cs, T)
    ((cn, _, Sn, _), (cg, _, Sg, model)), U0 = _both_paths(cs, T, N, 2.0, 0, ref)
    same_bits(f"{name} T{T}: generic states against fused", Sg, Sn)
    acc = np.zeros(N, f64)
    for t in range(T + 1):
        u = torch.from_numpy(U0[:, t]) if t < T else torch.zeros(N, cs["dc"])
        acc += model.cost(torch.from_numpy(Sg[:, t]).cuda(), u.cuda(), {"t": min(t, T - 1)}).cpu().numpy().astype(f64)
    same_bits(f"{name} T{T}: the generic path's stage costs, added in float64 and rounded once", acc.astype(f32), cn)
    c32, _, mag = TR.rollout(cs, ref, cs["angular"], U0)
    same_bits(f"{name} T{T}: fused against the restatement", cn, c32)
    c64 = TR.rollout(cs, ref, cs["angular"], U0, f64)[0]
    limit, yard = TR.band(c32, c64, mag)
    err = np.abs(cg.astype(f64) - c64)
    print(f"[mlp-track] {name} T{T} generic totals (torch.sum in fp32): ratio {err.max() / max(yard, 1e-300):.2f} of the fp32 band {yard:.3g}")
    assert np.all(err <= limit), f"{name}: {err.max():.3g}"


# ------------------------------------------------------------------------------ 7. opt-ins together, against the float64 solve
class TrackRef(sr.Model):
    """solve_ref.MlpModel with the tracking cost (tests/mlp_track_ref.py)"""

    def __init__(self, cs, ref):
        self.cs, self.ref, self.name, self.ds, self.dc = cs, ref, cs["model"], cs["DS"], cs["dc"]
        self.u_min, self.u_max, self.sigmas = f32(cs["u_min"]), f32(cs["u_max"]), f32(cs["sigmas"])

    def _run(self, x0, U, dtype):
        c, S, mag = TR.rollout(self.cs, self.ref, self.cs["angular"], U, dtype, x0=x0)
        return c, np.concatenate([S, np.zeros(S.shape[:2] + (self.ds - S.shape[2],), S.dtype)], axis=2), mag

    def rollout(self, x0, U, dtype=f64, states=None):
        c, S, mag = self._run(x0, U, dtype)
        band = TR.band(self._run(x0, U, f32)[0], c, mag)[0] if dtype == f64 else None
        return dict(costs=c, boundary=np.zeros(len(c), bool), scale=float(np.abs(c).max()), S=S, band=band)


def problem(cs, ref, T, N, lam, solver):
    pb = object.__new__(sr.Problem)
    pb.pair, pb.family, pb.model, pb.x0, pb.on = (), cs["model"], TrackRef(cs, ref), f32(cs["x0"]), set()
    pb.dc, pb.ds, pb.T, pb.N, pb.offset, pb.n, pb.inherit = cs["dc"], cs["DS"], T, N, 0, N, N
    pb.u_min, pb.u_max, pb.sigmas = f32(cs["u_min"]), f32(cs["u_max"]), f32(cs["sigmas"])
    pb.lams, pb.rule, pb.risk, pb.beta, pb.sg = (lam,) * 8, None, ("mean", 1), None, None
    pb.cov = dict(rate=float(solver._cov_rate), floor=float(solver._cov_floor), smin=f32(np.asarray(solver._sigma_min)),
                  smax=f32(np.asarray(solver._sigma_max)))
    pb.ac_weight = None
    return pb


@pytest.mark.parametrize("name", ["mlp42_tanh_2l_res", "mlp82_tanh_2l_res"])
def test_colored_noise_and_covariance_adaptation_with_a_reference(name):
    """noise_beta and adapt_covariance together with a reference and the angular components: three closed-loop forward() calls
    at N = 256, T = 8, every tick against solve_ref.tick on the device's own noise, at test_gpu_feature_pairs.TOL."""
    cs = TR.case(name)
    T, N = 8, 256
    ref = TR.reference(cs, T)
    solver, _ = build(cs, T, N, ref=ref, lam=LAM, noise_beta=0.9, adapt_covariance=True)
    x = x0_of(cs).cuda()
    for tick in range(3):
        mean = current_mean(solver)
        sigma = solver.sigma_seq.cpu().numpy()
        a, s = solver.forward(x)
        c, U = solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy()
        pb = problem(cs, ref, T, N, LAM, solver)
        carry = dict(t=tick, x=f32(x.cpu().numpy()), mean=mean, sigma=sigma, hist=None, tl=None)
        out = sr.tick(pb, carry, solver._action_noises.cpu().numpy(), given={"U": U, "costs": c, "lambda": LAM})
        tagname = f"{name} tick {tick}"
        same_bits(f"{tagname}: U", U, out["U_ref"])
        excess, left = sr.cost_excess(c, dict(out, limit=pb.model.limit))
        err_a, err_s = rel_err(a.cpu().numpy(), out["action"]), rel_err(s.cpu().numpy()[0], out["states"])
        err_t = float(np.max(np.abs(solver.sigma_seq.cpu().numpy().astype(f64) - out["sigma"]) / out["sigma"]))
        print(f"[mlp-track] {tagname}: costs {excess:.2f} of their band, action {err_a:.2e}, states {err_s:.2e}, sigma table "
              f"{err_t:.2e} (limit {TOL:g})")
        assert left == 0 and excess <= 1.0, tagname
        assert err_a < TOL and err_s < TOL and err_t < TOL, (tagname, err_a, err_s, err_t)
        x = s[0, 1].clone()


# ------------------------------------------------------------------------------ 8. a default handle is what it was
@pytest.mark.parametrize("N", [100, 4096, 4160])
@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("name", ["mlp41_tanh_2l_res", "mlp84_tanh_2l_res"])
def test_switched_off_again_equals_a_fresh_default_handle(name, math, N):
    """A fresh default MLP handle and one that had a reference and a mask, both switched off again: byte-identical costs,
    action_seq and state_seq — in the single launch (N <= 4096) and in the multi-kernel sequence."""
    cs = TR.case(name)
    T = cs["horizons"][-1]
    fresh, _ = build(cs, T, N, angular=(), lam=LAM)
    used, model = build(cs, T, N, ref=TR.reference(cs, T), lam=LAM)
    x0 = x0_of(cs).cuda()
    for s in (fresh, used):
        s.set_option("math", math)
    fresh.forward(x0)
    used.forward(x0)                      # one solve WITH the reference and the mask
    with_ref = used._costs.clone()
    assert not torch.equal(with_ref, fresh._costs)
    fresh.reset()
    used.reset()
    model.set_reference(None)
    model.set_angular(())
    for tick in range(2):
        a, s = fresh.forward(x0)
        b, r = used.forward(x0)
        assert torch.equal(a, b) and torch.equal(s, r) and torch.equal(fresh._costs, used._costs), (name, math, tick)
    n, mask = C.c_int(-1), C.c_uint32(99)
    used._h.call("mppi_get_mlp_reference", None, C.byref(n), 0, None)
    used._h.call("mppi_get_mlp_angular", C.byref(mask))
    assert (n.value, mask.value) == (0, 0)
