"""The 8-state learned-dynamics models (MPPI_MODEL_MLP81 / MLP82 / MLP84: envs.MLPModel8, mppi_set_mlp) on a real MI355X.

Costs and clamped actions come from the C ABI's individual entry points (test_gpu_action_cost.Rig); the references are the two
evaluations of tests/mlp8_ref.py on the EXPORTED actions.

  relu, math 0   every sample's cost equals the fp32 restatement bit for bit — by the rollout kernel with regenerated noise
                 and with tiles, by mppi_solve (the single launch up to 4096 samples), with fused_solve = 0 — and so do the
                 states of mppi_top_samples(8) and the returned state sequence.
  tanh / math 1  costs against the float64 evaluation inside mlp_ref.band: 4 x the distance of the numpy fp32 restatement from
                 float64 on the same actions, floored at 2 * 2^-24 * sum |terms of the cost| — the rule of the 4-state ids.
                 The measured ratio is printed as an `[mlp8]` line.
  mapping = 1    (the comparison kernel: a wavefront per trajectory) is held to the same band at every level.
Shapes: N in {64, 100, 4160} (one tile, a ragged tile, 65 tiles); T in {1, 4, 5, 8, 9} for mlp81 (four steps per float4
group), {1, 2, 3, 7, 8} for mlp82 and {1, 2, 3, 4, 5, 9} for mlp84 (ONE step per group: no native model walked that loop
before): the smallest that reach every copy of the horizon loop.

The generic path and the sum of the costs: the fused kernels add a trajectory's T + 1 stage costs in float64 and round once
(mppi_models.hpp: CostSum), the generic path adds the callables' stage costs as the reference does, torch.sum in fp32 — an
order that is not part of anybody's contract.  So "the same costs to the bit" is asked where it is defined: the state
sequences of every sample (no sum in them) at a real horizon, the per-stage costs of those states summed the fused way, and
the totals themselves at T = 1, where the sum is ONE exactly rounded addition on both paths.  The totals at the longer horizon
are held to the band.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import mlp8_ref as R
import solve_ref as sr
import stats_cases as sc
from helpers import rel_err
from test_gpu_action_cost import Rig, current_mean
from test_gpu_covariance import _need_gpu, weights64
from test_gpu_feature_pairs import TOL
from test_gpu_fused_geometry import took
from test_gpu_mlp_model import bits, check_top_states, same_bits

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
worst = {"ratio": 0.0}
LAM = 2.0


def model_of(cs, Ws=None, bs=None):
    from envs import MLPModel8

    P, ds = cs["params"], cs["ds"]
    return MLPModel8(cs["Ws"] if Ws is None else Ws, cs["bs"] if bs is None else bs, activation=cs["activation"],
                     residual=cs["residual"], goal=P[:ds], q=P[8:8 + ds], r=P[16:])


def build(cs, T, N, lam=1.0, tag=True, model=None, **kw):
    """(solver, model) around a case of the table; tag=False hides the native tags behind plain lambdas (generic path)."""
    _need_gpu()
    from pi_mpc.mppi import MPPI

    model = model_of(cs) if model is None else model
    if hasattr(model, "table"):
        assert np.array_equal(model.table, cs["table"]) and model.dim_state == 8
    dyn, cost = (model.dynamics, model.cost) if tag else ((lambda s, a: model.dynamics(s, a)), (lambda s, a, i: model.cost(s, a, i)))
    solver = MPPI(horizon=T, num_samples=N, dim_state=8, dim_control=cs["dc"], dynamics=dyn, cost_func=cost,
                  u_min=torch.tensor(cs["u_min"]), u_max=torch.tensor(cs["u_max"]), sigmas=torch.tensor(cs["sigmas"]),
                  lambda_=lam, **kw)
    assert (solver._model == cs["model"]) if tag else (solver._model is None)
    return solver, model


def x0_of(cs):
    return torch.from_numpy(cs["x0"].copy())


class Mlp8Rig(Rig):
    def __init__(self, cs, T, N, math=0, mode=None, **kw):
        self.cs = cs
        solver, self.mlp = build(cs, T, N, **kw)
        super().__init__(cs["model"], T, N, solver=(solver, x0_of(cs)))
        assert (self.ds, self.dc) == (8, cs["dc"])
        self.h.call("mppi_set_option", b"math", math)
        if mode is not None:
            self.h.call("mppi_set_option", b"fused_solve", mode)
        rng = np.random.default_rng(T * 1000 + N)
        self.mean0 = rng.uniform(f32(cs["u_min"]), f32(cs["u_max"]), (T, cs["dc"])).astype(f32)
        self.set_mean(self.mean0)

    def ref(self, U, dtype=f32, table=None, x0=None):
        cs = self.cs
        return R.rollout(cs["table"] if table is None else table, cs["params"], cs["hidden_layers"], cs["activation"],
                         cs["residual"], cs["x0"] if x0 is None else x0, U, dtype)

    def top_states(self, k, lam):
        st, w = torch.empty(k, self.T + 1, 8, device="cuda"), torch.empty(k, device="cuda")
        self.h.call("mppi_top_samples", k, float(lam), st.data_ptr(), w.data_ptr(), self.solver._stream())
        torch.cuda.synchronize()
        return st.cpu().numpy(), w.cpu().numpy()


def in_band(name, rig, c, U, refs=None):
    """-> the references (c32, c64, mag) of U, computed once per U and handed back in for the next cost vector"""
    if refs is None:
        c32, _, mag = rig.ref(U)
        refs = (c32, rig.ref(U, f64)[0], mag)
    c32, c64, mag = refs
    limit, yard = R.band(c32, c64, mag)
    err = np.abs(c.astype(f64) - c64)
    ratio = float(err.max() / yard) if yard > 0 else 0.0
    worst["ratio"] = max(worst["ratio"], ratio)
    print(f"[mlp8] {name}: ratio {ratio:.2f} of the fp32 band {yard:.3g}; max err {err.max():.3g}, largest so far {worst['ratio']:.2f}")
    assert np.all(np.isfinite(c)), name
    over = err > limit
    assert not over.any(), f"{name}: {int(over.sum())} costs beyond the band, worst {err.max():.3g} against {limit[np.argmax(err - limit)]:.3g}"
    return refs


RELU = [c[0] for c in R.CASES if c[3] == "relu"]
ALL = [c[0] for c in R.CASES]
PADDED = [c[0] for c in R.CASES if c[6] == 6]


def padding_stays_zero(name, cs, *state_arrays):
    for S in state_arrays:
        assert not np.asarray(S)[..., cs["ds"]:].any(), f"{name}: a padded state component is not exactly 0"


# ------------------------------------------------------------------------------ 1. relu, math 0: bit for bit
@pytest.mark.parametrize("name", RELU)
def test_relu_math0_costs_and_top_states_bit_for_bit(name):
    cs = R.case(name)
    for T in R.HORIZONS[cs["dc"]]:
        for N in R.SAMPLES:
            rig = Mlp8Rig(cs, T, N)
            tagname = f"{name} T{T} N{N}"
            c = rig.rollout(3)                       # the rollout kernel, noise regenerated in registers
            U = rig.actions_around(rig.mean0)
            c32, S32, _ = rig.ref(U)
            same_bits(f"{tagname} regenerated", c, c32)
            rig.h.call("mppi_set_option", b"noise_regen", 0)
            same_bits(f"{tagname} tiles", rig.rollout(3), c32)
            rig.h.call("mppi_set_option", b"noise_regen", 1)
            a, s, _, cs_ = rig.solve(3, LAM)         # mppi_solve: the single launch up to 4096 samples
            assert (took(rig.h) != (0, 0)) == (N <= 4096), tagname
            same_bits(f"{tagname} mppi_solve", cs_, c32)
            check_top_states(tagname, rig, c32, S32, LAM)
            top, _ = rig.top_states(8, LAM)
            same_bits(f"{tagname} state_seq of mppi_solve", s, rig.ref(a[None])[1][0])
            rig.set_mean(rig.mean0)                  # (the solve stored its own warm start)
            rig.h.call("mppi_set_option", b"fused_solve", 0)
            a0, s0, _, c0 = rig.solve(3, LAM)        # the multi-kernel sequence
            assert took(rig.h) == (0, 0), tagname
            same_bits(f"{tagname} fused_solve=0", c0, c32)
            check_top_states(f"{tagname} fused_solve=0", rig, c32, S32, LAM)
            same_bits(f"{tagname} state_seq, fused_solve=0", s0, rig.ref(a0[None])[1][0])
            padding_stays_zero(tagname, cs, s, s0, top)
            rig.close()


# ------------------------------------------------------------------------------ 2. tanh, and the fast level: the band
@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("name", ALL)
def test_costs_within_the_fp32_band_of_float64(name, math):
    cs = R.case(name)
    for T in R.HORIZONS[cs["dc"]]:
        for N in R.SAMPLES if T == R.HORIZONS[cs["dc"]][-1] else (64, 100):
            rig = Mlp8Rig(cs, T, N, math=math)
            tagname = f"{name} math {math} T{T} N{N}"
            c = rig.rollout(5)
            U = rig.actions_around(rig.mean0)
            refs = in_band(f"{tagname} rollout", rig, c, U)
            rig.h.call("mppi_set_option", b"noise_regen", 0)
            ct = rig.rollout(5)
            rig.h.call("mppi_set_option", b"noise_regen", 1)
            in_band(f"{tagname} tiles", rig, ct, U, refs)
            if N <= 4096:
                _, s1, _, c1 = rig.solve(5, LAM)
                assert took(rig.h) != (0, 0)
                in_band(f"{tagname} single launch", rig, c1, U, refs)
                rig.set_mean(rig.mean0)              # (the solve stored its own warm start)
                rig.h.call("mppi_set_option", b"fused_solve", 0)
                _, s0, _, c0 = rig.solve(5, LAM)
                assert took(rig.h) == (0, 0)
                in_band(f"{tagname} fused_solve=0", rig, c0, U, refs)
                padding_stays_zero(tagname, cs, s1, s0, rig.top_states(8, LAM)[0])
            rig.close()


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("name", ["mlp81_relu_2l_res", "mlp82_tanh_2l_abs", "mlp84_tanh_2l_res", "mlp84_relu_1l_abs_s6"])
def test_wavefront_per_trajectory_mapping(name, math):
    cs = R.case(name)
    for T in R.HORIZONS[cs["dc"]][-2:]:
        rig = Mlp8Rig(cs, T, 100, math=math)
        rig.h.call("mppi_set_option", b"mapping", 1)
        c = rig.rollout(6)
        in_band(f"{name} math {math} T{T} mapping 1", rig, c, rig.actions_around(rig.mean0))
        rig.close()


# ------------------------------------------------------------------------------ 3. against the generic path
def _both_paths(cs, T, N, lam, math):
    """The tagged solver and the same callables behind lambdas on the same injected noise -> per path (costs, U, states)"""
    x0 = x0_of(cs).cuda()
    rng = np.random.default_rng(9 + T)
    eps = torch.from_numpy((rng.standard_normal((N, T, cs["dc"])) * f32(cs["sigmas"])).astype(f32))
    outs = []
    for tag in (True, False):
        solver, model = build(cs, T, N, lam=lam, tag=tag)
        if tag:
            solver.set_option("math", math)
        solver.inject_noise(eps)
        solver.forward(x0)
        outs.append((solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy(),
                     solver._state_seq_batch.cpu().numpy(), model))
    U0 = np.clip(eps.numpy(), f32(cs["u_min"]), f32(cs["u_max"]))  # (first solve: zero warm start)
    assert np.array_equal(outs[0][1], U0) and np.array_equal(outs[1][1], U0)
    return outs, U0


@pytest.mark.parametrize("name", ["mlp81_relu_2l_res", "mlp82_relu_2l_abs", "mlp84_relu_2l_res", "mlp84_relu_1l_abs_s6",
                                  "mlp82_relu_1l_res"])
def test_generic_path_relu_math0_to_the_bit(name):
    """(the module's docstring says where the two paths' totals are comparable bit for bit, and why)"""
    cs = R.case(name)
    N = 100
    # T = 1: the totals themselves
    ((cn, _, Sn, _), (cg, _, Sg, _)), U0 = _both_paths(cs, 1, N, 2.0, 0)
    same_bits(f"{name} T1: generic costs against fused", cg, cn)
    same_bits(f"{name} T1: generic states against fused", Sg, Sn)
    same_bits(f"{name} T1: fused against the restatement", cn, R.rollout(cs["table"], cs["params"], cs["hidden_layers"], "relu",
                                                                          cs["residual"], cs["x0"], U0)[0])
    # a real horizon: every state of every sample, and the stage costs of the generic path's states summed the fused way
    T = R.HORIZONS[cs["dc"]][-1]
    ((cn, _, Sn, _), (cg, _, Sg, model)), U0 = _both_paths(cs, T, N, 2.0, 0)
    same_bits(f"{name} T{T}: generic states against fused", Sg, Sn)
    padding_stays_zero(name, cs, Sg, Sn)
    acc = np.zeros(N, f64)
    for t in range(T + 1):
        u = torch.from_numpy(U0[:, t]) if t < T else torch.zeros(N, cs["dc"])
        acc += model.cost(torch.from_numpy(Sg[:, t]).cuda(), u.cuda(), {}).cpu().numpy().astype(f64)
    same_bits(f"{name} T{T}: the generic path's stage costs, added in float64 and rounded once", acc.astype(f32), cn)
    c32, _, mag = R.rollout(cs["table"], cs["params"], cs["hidden_layers"], "relu", cs["residual"], cs["x0"], U0)
    same_bits(f"{name} T{T}: fused against the restatement", cn, c32)
    c64 = R.rollout(cs["table"], cs["params"], cs["hidden_layers"], "relu", cs["residual"], cs["x0"], U0, f64)[0]
    limit, yard = R.band(c32, c64, mag)
    err = np.abs(cg.astype(f64) - c64)
    print(f"[mlp8] {name} T{T} generic totals (torch.sum in fp32): ratio {err.max() / max(yard, 1e-300):.2f} of the fp32 band {yard:.3g}")
    assert np.all(err <= limit), f"{name}: {err.max():.3g}"


@pytest.mark.parametrize("name,math", [("mlp81_tanh_2l_res", 0), ("mlp82_tanh_2l_abs", 1), ("mlp84_tanh_2l_res", 0),
                                       ("mlp84_tanh_2l_abs", 1), ("mlp84_relu_2l_res", 1), ("mlp82_tanh_2l_res_s6", 1)])
def test_generic_path_within_the_band(name, math):
    cs = R.case(name)
    T, N = R.HORIZONS[cs["dc"]][-1], 600
    ref = lambda U, dtype: R.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"],  # noqa: E731
                                     cs["x0"], U, dtype)
    ((cn, _, Sn, _), (cg, _, Sg, _)), U0 = _both_paths(cs, T, N, 2.0, math)
    (c32, _, mag), (c64, S64, _) = ref(U0, f32), ref(U0, f64)
    limit, yard = R.band(c32, c64, mag)
    for label, c in (("native", cn), ("generic", cg)):
        err = np.abs(c.astype(f64) - c64)
        print(f"[mlp8] {name} math {math} {label} path costs: ratio {err.max() / max(yard, 1e-300):.2f} of the fp32 band {yard:.3g}")
        assert np.all(err <= limit), f"{name} {label}: {err.max():.3g}"
    assert np.max(np.abs(Sn - S64)) <= 1e-5 and np.max(np.abs(Sg - S64)) <= 1e-5
    padding_stays_zero(name, cs, Sn, Sg)


# ------------------------------------------------------------------------------ 4. forward() against the float64 solve
class Mlp8Ref(sr.Model):
    """solve_ref.MlpModel for the 8-state ids (tests/mlp8_ref.py)"""

    def __init__(self, cs):
        self.cs, self.name, self.ds, self.dc = cs, cs["model"], 8, cs["dc"]
        self.u_min, self.u_max, self.sigmas = f32(cs["u_min"]), f32(cs["u_max"]), f32(cs["sigmas"])

    def _run(self, x0, U, dtype):
        cs = self.cs
        return R.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], x0, U, dtype)

    def rollout(self, x0, U, dtype=f64, states=None):
        c, S, mag = self._run(x0, U, dtype)
        band = R.band(self._run(x0, U, f32)[0], c, mag)[0] if dtype == f64 else None
        return dict(costs=c, boundary=np.zeros(len(c), bool), scale=float(np.abs(c).max()), S=S, band=band)


def problem(cs, T, N, lam, solver):
    """A solve_ref.Problem of this module's shapes (solve_ref.Shape fixes those of the feature pairs): the features the solver
    was built with, read from the solver"""
    pb = object.__new__(sr.Problem)
    pb.pair, pb.family, pb.model, pb.x0, pb.on = (), cs["model"], Mlp8Ref(cs), f32(cs["x0"]), set()
    pb.dc, pb.ds, pb.T, pb.N, pb.offset, pb.n, pb.inherit = cs["dc"], 8, T, N, 0, N, N
    pb.u_min, pb.u_max, pb.sigmas = f32(cs["u_min"]), f32(cs["u_max"]), f32(cs["sigmas"])
    pb.lams, pb.rule, pb.risk, pb.beta, pb.sg = (lam,) * 8, None, ("mean", 1), None, None
    pb.cov = None
    if solver._adapt_covariance:
        pb.cov = dict(rate=float(solver._cov_rate), floor=float(solver._cov_floor), smin=f32(np.asarray(solver._sigma_min)),
                      smax=f32(np.asarray(solver._sigma_max)))
    pb.ac_weight = float(solver._action_cost_weight) if solver._action_cost else None
    return pb


SOLVER_CASES = [("fixed", dict(lam=LAM)), ("essps", dict(lam="ESSPS", essps_target_ess=40.0, lambda_min=1e-3, lambda_max=1e5)),
                ("ac_cov", dict(lam=LAM, action_cost=True, adapt_covariance=True))]


@pytest.mark.parametrize("rule,kw", SOLVER_CASES, ids=[c[0] for c in SOLVER_CASES])
@pytest.mark.parametrize("name", ["mlp82_tanh_2l_res", "mlp84_tanh_2l_res"])
def test_forward_against_the_float64_solve(name, rule, kw):
    """Three closed-loop forward() calls at N = 256, T = 8; every tick against solve_ref.tick (the float64 restatement of a
    whole tick) on the device's own noise, U, costs and temperature, at test_gpu_feature_pairs.TOL."""
    cs = R.case(name)
    T, N = 8, 256
    solver, _ = build(cs, T, N, **kw)
    x = x0_of(cs).cuda()
    for tick in range(3):
        mean = current_mean(solver)
        sigma = solver.sigma_seq.cpu().numpy()
        lam_term = LAM if rule != "essps" else (float(solver._last_lambda) if tick else 0.0)
        a, s = solver.forward(x)
        c, U = solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy()
        lam = float(solver._last_lambda)
        if rule == "essps":
            ess = weights64(c, lam)[1]
            print(f"[mlp8] {name} essps tick {tick}: lambda {lam:.6g}, ESS {ess:.3f} (target 40)")
            assert 1e-3 < lam < 1e5 and abs(ess - 40.0) / 40.0 <= sc.ESS_BAND, (name, tick, lam, ess)
        else:
            assert lam == LAM
        pb = problem(cs, T, N, lam_term if rule == "essps" else lam, solver)
        carry = dict(t=tick, x=f32(x.cpu().numpy()), mean=mean, sigma=sigma, hist=None, tl=None)
        ref = sr.tick(pb, carry, solver._action_noises.cpu().numpy(), given={"U": U, "costs": c, "lambda": lam})
        tagname = f"{name} {rule} tick {tick}"
        same_bits(f"{tagname}: U", U, ref["U_ref"])
        excess, left = sr.cost_excess(c, dict(ref, limit=pb.model.limit))
        err_a, err_s = rel_err(a.cpu().numpy(), ref["action"]), rel_err(s.cpu().numpy()[0], ref["states"])
        print(f"[mlp8] {tagname}: costs {excess:.2f} of their band, action {err_a:.2e}, states {err_s:.2e} (limit {TOL:g})")
        assert left == 0 and excess <= 1.0, tagname
        assert err_a < TOL and err_s < TOL, (tagname, err_a, err_s)
        if pb.cov is not None:
            err_t = float(np.max(np.abs(solver.sigma_seq.cpu().numpy().astype(f64) - ref["sigma"]) / ref["sigma"]))
            print(f"[mlp8] {tagname}: sigma table {err_t:.2e}")
            assert err_t < TOL, (tagname, err_t)
            if tick:
                assert np.any(mean != 0) and not np.array_equal(sigma, np.tile(f32(cs["sigmas"]), (T, 1)))
        x = s[0, 1].clone()


@pytest.mark.parametrize("name", ["mlp82_tanh_2l_res", "mlp84_tanh_2l_res"])
def test_colored_noise_matches_its_materialised_twin(name):
    """tests/test_gpu_colored_noise.py's statement: three closed-loop solves with noise_beta = 0.9; in lockstep a default solver
    into which each solve's exported colored noise is injected returns the same bits."""
    cs = R.case(name)
    (a, _), (b, _) = build(cs, 8, 256, lam=LAM, noise_beta=0.9), build(cs, 8, 256, lam=LAM)
    x = x0_of(cs).cuda()
    for tick in range(3):
        act, seq = a.forward(x)
        assert took(a._h) == (0, 0)
        b.inject_noise(a._action_noises)
        act_b, seq_b = b.forward(x)
        assert torch.equal(act, act_b) and torch.equal(seq, seq_b) and torch.equal(a._costs, b._costs), tick
        (sa, wa), (sb, wb) = a.get_top_samples(8), b.get_top_samples(8)
        assert torch.equal(sa, sb) and torch.equal(wa, wb), tick
        assert torch.isfinite(act).all() and torch.isfinite(seq).all()
        x = seq[0, 1].clone()
    z = a._action_noises.cpu().numpy() / f32(cs["sigmas"])
    assert np.corrcoef(z[:, :-1].ravel(), z[:, 1:].ravel())[0, 1] > 0.8  # (the filter is on)


# ------------------------------------------------------------------------------ 5. particles and ensembles
PARTS = (R.X0[None, :] + f32([[0.0] * 8, [0.1, -0.05, 0.02, 0.03, -0.02, 0.04, 0.01, -0.03],
                              [-0.2, 0.1, 0.05, -0.1, 0.03, -0.06, 0.02, 0.05]])).astype(f32)


def member_nets(cs, n=3):
    return [R.make_net(500 + e, cs["dc"], cs["hidden_layers"], cs["activation"], cs["residual"]) for e in range(n)]


def plain_costs(cs, model, x, T, N):
    """The first solve of a fresh plain solver around `model` from x, math level 0 -> costs"""
    solver, _ = build(dict(cs, table=model.table), T, N, lam=LAM, model=model)
    solver.set_option("math", 0)
    solver.forward(torch.from_numpy(np.ascontiguousarray(x, f32)).cuda())
    return solver._costs.cpu().numpy()


@pytest.mark.parametrize("name", ["mlp81_relu_2l_res", "mlp82_tanh_2l_abs", "mlp84_relu_2l_res", "mlp84_tanh_1l_res"])
def test_particles_and_ensemble_rows_equal_plain_solves(name):
    from envs import MLPEnsemble

    cs = R.case(name)
    T, N = 5, 100
    # state particles: row m is the plain solve from particle m
    solver, model = build(cs, T, N, lam=LAM, risk="worst")
    solver.set_option("math", 0)
    solver.set_state_particles(torch.from_numpy(PARTS))
    solver.forward(x0_of(cs).cuda())
    M = solver.particle_costs.cpu().numpy()
    assert M.shape == (3, N) and np.all(np.isfinite(M))
    for m in range(3):
        same_bits(f"{name}: particle {m}", M[m], plain_costs(cs, model, PARTS[m], T, N))
    same_bits(f"{name}: the fold", solver._costs.cpu().numpy(), M.max(0))
    assert not np.array_equal(M[0], M[1])
    # an ensemble of three MLPModel8 members: one particle per network, from the nominal state ...
    members = [model_of(cs, Ws, bs) for Ws, bs in member_nets(cs)]
    ens = MLPEnsemble(members, nominal=1)
    assert ens.model_name == cs["model"] and ens.tables.shape == (3, R.n_floats(cs["dc"]))
    es, _ = build(cs, T, N, lam=LAM, model=ens, risk="mean")
    es.set_option("math", 0)
    es.set_model_particles("all")
    a, s = es.forward(x0_of(cs).cuda())
    assert es.particle_members == (0, 1, 2)
    E = es.particle_costs.cpu().numpy()
    rows = [plain_costs(cs, members[m], cs["x0"], T, N) for m in range(3)]
    for m in range(3):
        same_bits(f"{name}: member {m} from the nominal state", E[m], rows[m])
    assert not np.array_equal(E[0], E[1]) and not np.array_equal(E[1], E[2])
    # (the returned state sequence is the nominal member's)
    _, Sa, _ = R.rollout(members[1].table, cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], cs["x0"],
                         a.cpu().numpy()[None], f64)
    assert np.max(np.abs(s.cpu().numpy()[0] - Sa[0])) <= 1e-5
    # ... and with a particle table of its own: row m is member m from particle m
    es2, _ = build(cs, T, N, lam=LAM, model=MLPEnsemble([copy.deepcopy(m) for m in members]), risk="mean")
    es2.set_option("math", 0)
    es2.set_state_particles(torch.from_numpy(PARTS), members=[2, 0, 1])
    es2.forward(x0_of(cs).cuda())
    E2 = es2.particle_costs.cpu().numpy()
    for m, e in enumerate((2, 0, 1)):
        same_bits(f"{name}: member {e} from particle {m}", E2[m], plain_costs(cs, members[e], PARTS[m], T, N))


# ------------------------------------------------------------------------------ 6. the table between solves, copies
def test_update_weights_between_two_solves():
    cs, cs2 = R.case("mlp84_relu_2l_res"), R.case("mlp84_relu_2l_abs")
    rig = Mlp8Rig(cs, 9, 4160)
    c = rig.rollout(3)
    U = rig.actions_around(rig.mean0)
    same_bits("before", c, rig.ref(U)[0])
    Ws2 = [w.copy() for w in cs2["Ws"]]
    Ws2[-1] = (Ws2[-1] * f32(0.05)).astype(f32)  # (residual stays on: keep the step small)
    rig.mlp.update_weights(Ws2, cs2["bs"])
    assert rig.mlp.version == 1
    rig.solver._refresh_model_inputs()              # what every forward() does first
    c2 = rig.rollout(3)
    table2 = R.pack(Ws2, cs2["bs"], 4)
    same_bits("after update_weights", c2, rig.ref(U, table=table2)[0])
    assert not np.array_equal(c, c2)
    rig.close()
    # ... and through forward(): two solves, new weights in between, each against its own table
    solver, model = build(cs, 9, 600, lam=2.0)
    x0 = x0_of(cs).cuda()
    solver.set_option("math", 0)
    solver.forward(x0)
    c1, U1 = solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy()
    same_bits("forward 1", c1, R.rollout(cs["table"], cs["params"], 2, "relu", True, cs["x0"], U1)[0])
    model.update_weights(Ws2, cs2["bs"])
    solver.forward(x0)
    c2, U2 = solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy()
    same_bits("forward 2", c2, R.rollout(table2, cs["params"], 2, "relu", True, cs["x0"], U2)[0])


def test_deep_copy_and_state_dict_round_trip():
    cs = R.case("mlp84_tanh_2l_abs")
    solver, model = build(cs, 9, 1000, lam=2.0)
    x0 = x0_of(cs).cuda()
    solver.forward(x0)
    twin = copy.deepcopy(solver)
    assert twin._cost_owner is not model and type(twin._cost_owner) is type(model) and twin._model == "mlp84"
    for tick in range(3):
        a, s = solver.forward(x0)
        b, r = twin.forward(x0)
        assert torch.equal(a, b) and torch.equal(s, r) and torch.equal(solver._costs, twin._costs), tick
    sd = solver.state_dict()
    assert "_extra_state" in sd
    other, _ = build(cs, 9, 1000, lam=2.0)
    other.load_state_dict(sd)
    a, s = solver.forward(x0)
    b, r = other.forward(x0)
    assert torch.equal(a, b) and torch.equal(s, r) and torch.equal(solver._costs, other._costs)


# ------------------------------------------------------------------------------ 7. what the C ABI refuses
def test_c_abi_refusals():
    _need_gpu()
    from mppi_playground_amd import _capi

    handles = {}
    for dc in (1, 2, 4):
        cs = R.case(f"mlp8{dc}_relu_2l_res")
        cfg = _capi.MppiConfig()
        cfg.model, cfg.horizon, cfg.dim_state, cfg.dim_control = _capi.MODEL_IDS[f"mlp8{dc}"], 5, 8, dc
        cfg.num_samples, cfg.sample_offset, cfg.inherit_count = 100, 0, 100
        for k in range(dc):
            cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = cs["u_min"][k], cs["u_max"][k], cs["sigmas"][k]
        cfg.seed, cfg.device = 1, 0
        h = handles[dc] = _capi.Handle(cfg)
        par = np.ascontiguousarray(cs["params"], f32)
        for n in (16, 19, 8 + dc, 16 + dc - 1, 16 + dc + 1):  # wrong parameter counts (the 4-state id's among them)
            with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
                h.call("mppi_set_model_params", np.zeros(32, f32).ctypes.data_as(C.c_void_p), n)
        h.call("mppi_set_model_params", par.ctypes.data_as(C.c_void_p), 16 + dc)
        x0 = x0_of(cs).cuda()
        h.call("mppi_set_state", x0.data_ptr(), 1, None)
        h.call("mppi_sample", 1, None)
        with pytest.raises(_capi.MppiError, match=r"\(-3\).*weight table"):  # MPPI_E_STATE: no table yet
            h.call("mppi_rollout_cost", None)
        with pytest.raises(_capi.MppiError, match=r"\(-3\)"):
            h.call("mppi_solve", None, 1, 1.0, None, None, None, None)
        tab = np.ascontiguousarray(cs["table"], f32)
        with pytest.raises(_capi.MppiError, match=r"\(-3\)"):                # a member before any table
            h.call("mppi_set_mlp_member", 0, tab.ctypes.data_as(C.c_void_p), int(tab.size), None)
        big = np.zeros(2048, f32)
        big[:tab.size] = tab
        put = lambda n, hl=2, act=0, res=1: h.call("mppi_set_mlp", big.ctypes.data_as(C.c_void_p), n, hl, act, res, None)  # noqa: E731
        wrong = {tab.size - 1, tab.size + 1, 0, 1380 if dc == 1 else 1412} | {R.n_floats(o) for o in (1, 2, 4) if o != dc}
        for n in sorted(wrong):   # wrong lengths: the other ids', the 4-state ids'
            with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
                put(n)
            with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
                h.call("mppi_set_mlp_ensemble", big.ctypes.data_as(C.c_void_p), 1, n, 2, 0, 1, 0, None)
        for bad in (np.nan, np.inf):
            big[tab.size - 1] = bad
            with pytest.raises(_capi.MppiError, match=r"\(-1\).*finite"):
                put(int(tab.size))
        big[tab.size - 1] = tab[-1]
        for kw in (dict(hl=0), dict(hl=3), dict(act=2), dict(res=2)):
            with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
                put(int(tab.size), **kw)
        put(int(tab.size))
        h.call("mppi_rollout_cost", None)                # now it runs
        c = torch.empty(100, device="cuda")
        h.call("mppi_get_costs", c.data_ptr(), 1, None)
        torch.cuda.synchronize()
        U = torch.empty(100, 5, dc, device="cuda")
        h.call("mppi_export_noise", None, U.data_ptr(), None)
        torch.cuda.synchronize()
        want = R.rollout(cs["table"], cs["params"], 2, "relu", True, cs["x0"], U.cpu().numpy())[0]
        h.call("mppi_set_option", b"math", 0)
        h.call("mppi_rollout_cost", None)
        h.call("mppi_get_costs", c.data_ptr(), 1, None)
        torch.cuda.synchronize()
        same_bits(f"mlp8{dc} through the bare C ABI", c.cpu().numpy(), want)
        with pytest.raises(_capi.MppiError, match=r"\(-1\)"):  # no reference window on these handles
            h.call("mppi_set_reference", np.zeros(40, f32).ctypes.data_as(C.c_void_p), 10, None)
        # mppi_model_step keeps refusing the learned-dynamics ids
        s, a = torch.zeros(8, device="cuda"), torch.zeros(4, device="cuda")
        rc = h.lib.mppi_model_step(_capi.MODEL_IDS[f"mlp8{dc}"], par.ctypes.data_as(C.c_void_p), 16 + dc, None, None, s.data_ptr(),
                                   a.data_ptr(), s.data_ptr(), None, 0.0, None, None)
        assert rc == -1
    # a 4-state handle refuses an 8-state table and the other way round; another model's handle refuses both
    import mlp_ref as R4
    from test_gpu_covariance import make
    from test_gpu_mlp_model import build as build4

    s4, _ = build4(R4.case("mlp42_relu_2l_res"), 7, 64)
    t8 = np.ascontiguousarray(R.case("mlp82_relu_2l_res")["table"], f32)
    with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
        s4._h.call("mppi_set_mlp", t8.ctypes.data_as(C.c_void_p), int(t8.size), 2, 0, 1, None)
    pend, _ = make("pendulum", 8, 64, 1.0)
    with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
        pend._h.call("mppi_set_mlp", t8.ctypes.data_as(C.c_void_p), int(t8.size), 2, 0, 1, None)
    for h in handles.values():
        h.close()
    # the Python helper refuses wrong dims before anything reaches the device
    with pytest.raises(AssertionError):                  # a 2-control model on a 4-control solver
        build(dict(R.case("mlp82_relu_2l_res"), dc=4, **R.LIMITS[4]), 5, 64)
