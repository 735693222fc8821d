"""The learned terminal value of the learned-dynamics models (mppi_set_mlp_value; envs.MLPModel.set_value / terminal_cost) and
the solver keyword MPPI(..., terminal_cost=) on a real MI355X.

Costs and clamped actions come from the C ABI's individual entry points (test_gpu_action_cost.Rig); the reference is the numpy
restatement of tests/mlp_value_ref.py on the EXPORTED actions (tests/test_mlp_value_host.py holds it to the torch callable and
to the functor compiled for the host, on final states that make hidden units of both signs).

  relu, math 0   every sample's cost equals the restatement bit for bit: the rollout kernel with regenerated noise and with
                 tiles, mppi_solve in the single launch (N <= 4096) and with fused_solve = 0; a value alone (which must select
                 the instantiation that carries it) and reference + mask + value; the costs do NOT equal the restatement
                 without the value.
  the band       tanh value networks, math 1 and mapping = 1 inside mlp_ref.band (4 x the fp32 restatement's own distance
                 from float64, floored at 2 * 2^-24 * sum |terms|); the measured ratio is printed as a `[mlp-value]` line.
Shapes: N in {64, 100, 4160} (one tile, a ragged tile, 65 tiles), T from HORIZONS of the two case tables (they start at 1).
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import action_cost_ref as acref
import mlp_track_ref as TR
import mlp_value_ref as VR
from helpers import rel_err
from test_gpu_action_cost import Rig, term
from test_gpu_covariance import _need_gpu, make
from test_gpu_feature_pairs import TOL
from test_gpu_fused_geometry import took
from test_gpu_mlp_model import same_bits
from test_gpu_mlp_tracking import _raw_handle, _vp, model_of, put_reference, x0_of

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
worst = {"ratio": 0.0}
LAM = 2.0
ONE_PER_ID = ["mlp41_relu_2l_res", "mlp42_relu_1l_abs", "mlp81_relu_2l_res_s6", "mlp82_relu_2l_res", "mlp84_relu_1l_abs"]
VALUES = [(1, 32), (2, 32), (2, 20), (1, 7)]  # (hidden layers, width) of the value networks


def value_for(cs, k, activation, scale=1.0):
    hidden, width = VALUES[k % len(VALUES)]
    return VR.make_value(k + 10 * len(cs["name"]), cs["ds"], hidden, activation, width, scale)


def build(cs, T, N, val, ref=None, angular=(), lam=1.0, tag=True, model=None, weight=1.0, replace=False, terminal=True, **kw):
    """(solver, model) around a case with a value network; tag=False hides the native tags of all three callables."""
    _need_gpu()
    from pi_mpc.mppi import MPPI

    model = model_of(cs, angular) if model is None else model
    if ref is not None:
        put_reference(model, cs, ref)
    if val is not None:
        model.set_value(val["Ws"], val["bs"], activation=val["activation"], weight=weight, replace_terminal=replace)
    if tag:
        dyn, cost, trm = model.dynamics, model.cost, model.terminal_cost
    else:
        dyn, cost, trm = (lambda s, a: model.dynamics(s, a)), (lambda s, a, i: model.cost(s, a, i)), (lambda s: model.terminal_cost(s))
    solver = MPPI(horizon=T, num_samples=N, dim_state=cs["DS"], dim_control=cs["dc"], dynamics=dyn, cost_func=cost,
                  terminal_cost=trm if terminal else None, u_min=torch.tensor(cs["u_min"]), u_max=torch.tensor(cs["u_max"]),
                  sigmas=torch.tensor(cs["sigmas"]), lambda_=lam, **kw)
    assert (solver._model == cs["model"]) if tag else (solver._model is None)
    return solver, model


class ValueRig(Rig):
    def __init__(self, cs, T, N, val, ref=None, angular=(), math=0, weight=1.0, replace=False, **kw):
        self.cs, self.val, self.table, self.angular, self.weight, self.replace = cs, val, ref, angular, weight, replace
        solver, self.mlp = build(cs, T, N, val, ref=ref, angular=angular, weight=weight, replace=replace, **kw)
        super().__init__(cs["model"], T, N, solver=(solver, x0_of(cs)))
        self.h.call("mppi_set_option", b"math", math)
        rng = np.random.default_rng(T * 1000 + N)
        self.mean0 = rng.uniform(f32(cs["u_min"]), f32(cs["u_max"]), (T, cs["dc"])).astype(f32)
        self.set_mean(self.mean0)

    def new_value(self, val, weight=1.0, replace=False):
        self.val, self.weight, self.replace = val, weight, replace
        self.mlp.set_value(val["Ws"], val["bs"], activation=val["activation"], weight=weight, replace_terminal=replace)
        self.solver._refresh_model_inputs()  # what every forward() does first

    def ref(self, U, dtype=f32, val="own", **kw):
        return VR.rollout(self.cs, self.val if isinstance(val, str) else val, U, dtype, ref=self.table, angular=self.angular,
                          weight=self.weight, replace_terminal=self.replace, **kw)

    def four_paths(self, idx=3):
        """(name, costs) of the regenerating rollout, tiles, mppi_solve and fused_solve = 0 on the noise of solve `idx`."""
        out = [("regenerated", self.rollout(idx))]
        self.h.call("mppi_set_option", b"noise_regen", 0)
        out.append(("tiles", self.rollout(idx)))
        self.h.call("mppi_set_option", b"noise_regen", 1)
        self.set_mean(self.mean0)
        out.append(("mppi_solve", self.solve(idx, LAM)[3]))
        assert (took(self.h) != (0, 0)) == (self.N <= 4096)
        self.set_mean(self.mean0)                  # (the solve stored its own warm start)
        self.h.call("mppi_set_option", b"fused_solve", 0)
        out.append(("fused_solve=0", self.solve(idx, LAM)[3]))
        assert took(self.h) == (0, 0)
        self.h.call("mppi_set_option", b"fused_solve", 1)
        self.set_mean(self.mean0)
        return out


def in_band(name, rig, c, U, refs=None):
    if refs is None:
        c32, _, mag = rig.ref(U)
        refs = (c32, rig.ref(U, f64)[0], mag)
    c32, c64, mag = refs
    limit, yard = VR.band(c32, c64, mag)
    err = np.abs(c.astype(f64) - c64)
    ratio = float(err.max() / yard) if yard > 0 else 0.0
    worst["ratio"] = max(worst["ratio"], ratio)
    print(f"[mlp-value] {name}: ratio {ratio:.2f} of the fp32 band {yard:.3g}; max err {err.max():.3g}, largest so far {worst['ratio']:.2f}")
    assert np.all(np.isfinite(c)), name
    over = err > limit
    assert not over.any(), f"{name}: {int(over.sum())} costs beyond the band, worst {err.max():.3g} against {limit[np.argmax(err - limit)]:.3g}"
    return refs


# ------------------------------------------------------------------------------ 1. relu, math 0: bit for bit
@pytest.mark.parametrize("name", ONE_PER_ID)
def test_relu_math0_costs_bit_for_bit(name):
    """Per (T, N): a handle with a value ALONE and one with reference + mask + value; on each, two of the eight settings
    (value network of one / two hidden layers and two widths, replace_terminal off / on), so that every id sees every setting."""
    cs = TR.case(name)
    turn = 0
    seen = set()
    for T in cs["horizons"]:
        for N in TR.SAMPLES:
            for ref, angular in ((None, ()), (TR.reference(cs, T), cs["angular"])):
                rig = None
                for _ in range(2):
                    k, replace = turn % len(VALUES), (turn // len(VALUES)) % 2 == 1
                    turn += 1
                    seen.add((VALUES[k][0], replace, ref is None))
                    val = value_for(cs, k, "relu")
                    if rig is None:
                        rig = ValueRig(cs, T, N, val, ref=ref, angular=angular, weight=0.75, replace=replace)
                    else:
                        rig.new_value(val, weight=0.75, replace=replace)
                    tagname = f"{name} T{T} N{N} value {VALUES[k]} replace {replace} {'alone' if ref is None else 'ref+mask'}"
                    paths = rig.four_paths()
                    U = rig.actions_around(rig.mean0)
                    c32 = rig.ref(U)[0]
                    without = rig.ref(U, val=None)[0]
                    assert not np.array_equal(c32, without), tagname
                    for path, c in paths:
                        same_bits(f"{tagname} {path}", c, c32)
                        assert not np.array_equal(c, without), (tagname, path)  # (the value is in these costs)
                rig.close()
    assert seen == {(h, r, a) for h in (1, 2) for r in (False, True) for a in (False, True)}


# ------------------------------------------------------------------------------ 2. the band: tanh, math 1, mapping 1
@pytest.mark.parametrize("name,math", [("mlp41_tanh_2l_res", 0), ("mlp41_tanh_2l_res", 1), ("mlp42_relu_1l_abs", 1), ("mlp81_tanh_1l_abs", 1),
                                       ("mlp82_tanh_2l_res_s6", 0), ("mlp82_tanh_2l_res_s6", 1), ("mlp84_tanh_2l_res", 1)])
def test_costs_within_the_fp32_band_of_float64(name, math):
    cs = TR.case(name)
    turn = 0
    for T in cs["horizons"]:
        for N in TR.SAMPLES if T == cs["horizons"][-1] else (100,):
            k, replace, with_ref = turn % len(VALUES), (turn // 2) % 2 == 1, turn % 3 == 0
            turn += 1
            rig = ValueRig(cs, T, N, value_for(cs, k, "tanh"), ref=TR.reference(cs, T) if with_ref else None,
                           angular=cs["angular"] if with_ref else (), math=math, weight=1.5, replace=replace)
            tagname = f"{name} math {math} T{T} N{N} value {VALUES[k]} replace {replace} ref {with_ref}"
            paths = rig.four_paths(5) if N <= 4096 else [("regenerated", rig.rollout(5))]
            U = rig.actions_around(rig.mean0)
            refs = None
            for path, c in paths:
                refs = in_band(f"{tagname} {path}", rig, c, U, refs)
            rig.h.call("mppi_set_option", b"mapping", 1)   # a wavefront per trajectory: lane T carries the value
            in_band(f"{tagname} mapping 1", rig, rig.rollout(5), U, refs)
            rig.close()


@pytest.mark.parametrize("name", ONE_PER_ID)
def test_wavefront_per_trajectory_mapping_relu(name):
    """mapping = 1 sums the T + 1 costs in another order (a shuffle tree in fp32): the band."""
    cs = TR.case(name)
    for T, replace in ((1, True), (cs["horizons"][1], True), (cs["horizons"][-1], False)):
        rig = ValueRig(cs, T, 100, value_for(cs, 1, "relu"), weight=0.5, replace=replace)
        rig.h.call("mppi_set_option", b"mapping", 1)
        c = rig.rollout(6)
        U = rig.actions_around(rig.mean0)
        in_band(f"{name} T{T} mapping 1 relu", rig, c, U)
        assert not np.array_equal(c, rig.ref(U, val=None)[0])
        rig.close()


# ------------------------------------------------------------------------------ 3. the control-cost instantiation
@pytest.mark.parametrize("name", ONE_PER_ID)
def test_action_cost_rollout_carries_the_value(name):
    """rollout_action_cost_kernel, regenerated noise and tiles: the cost with the value (bit for bit at math 0 with weight 0 of
    the TERM) plus the term, against tests/action_cost_ref.py on top of the restatement."""
    cs = TR.case(name)
    for T in cs["horizons"][-2:]:
        for N in (100, 4160):
            rig = ValueRig(cs, T, N, value_for(cs, 2, "relu"), weight=0.75, action_cost=True)
            tagname = f"{name} T{T} N{N} action_cost"
            g = acref.g32(rig.mean0, rig.solver._sigmas.cpu().numpy())
            rig.h.call("mppi_sample", 4, rig.solver._stream())
            U = rig.actions_around(rig.mean0)
            c32 = rig.ref(U)[0]
            assert not np.array_equal(c32, rig.ref(U, val=None)[0])
            for regen in (1, 0):
                rig.h.call("mppi_set_option", b"noise_regen", regen)
                term(rig, 0.0, LAM)
                same_bits(f"{tagname} regen {regen} weight 0", rig.rollout(4), c32)
                term(rig, 1.0, LAM)
                c1 = rig.rollout(4)
                acref.check(f"{tagname} regen {regen}", c1, c32, acref.kappa32(1.0, LAM), g, U)
            rig.close()


# ------------------------------------------------------------------------------ 4. particles and ensembles
def plain_costs(cs, model, x, T, N):
    """The first solve of a fresh plain solver around a copy of `model` (its table, its value) from x, math 0 -> costs"""
    solver, _ = build(cs, T, N, None, lam=LAM, model=copy.deepcopy(model))
    solver.set_option("math", 0)
    solver.forward(torch.from_numpy(np.ascontiguousarray(x, f32)).cuda())
    return solver._costs.cpu().numpy()


@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp82_relu_2l_res", "mlp84_tanh_1l_abs"])
def test_particle_rows_equal_plain_handles(name):
    """P = 3 state particles on one model, and through E = 3 members of an ensemble that shares ONE value: row m of
    particle_costs is what a plain handle holding member members[m]'s table and the same value computes from particles[m]."""
    from envs import MLPEnsemble

    cs = TR.case(name)
    R = TR.module_of(name)
    N, T = 100, cs["horizons"][-1]
    parts = np.stack([f32(cs["x0"]) + f32(0.1 * j) * f32(np.resize([1.0, -0.5, 0.25, 0.3], cs["DS"])) for j in range(3)]).astype(f32)
    parts[:, cs["ds"]:] = 0
    val = value_for(cs, 1, "relu" if "_relu_" in name else "tanh")
    # one model, three start states
    solver, model = build(cs, T, N, val, lam=LAM, weight=0.75, risk="mean")
    solver.set_option("math", 0)
    solver.set_state_particles(torch.from_numpy(parts))
    solver.forward(x0_of(cs).cuda())
    E = solver.particle_costs.cpu().numpy()
    assert E.shape == (3, N) and np.all(np.isfinite(E))
    U = solver._perturbed_action_seqs.cpu().numpy()
    for m in range(3):
        same_bits(f"{name}: particle {m}", E[m], plain_costs(cs, model, parts[m], T, N))
        if "_relu_" in name:
            same_bits(f"{name}: particle {m} against the restatement", E[m], VR.rollout(cs, val, U, weight=0.75, x0=parts[m])[0])
            assert not np.array_equal(E[m], VR.rollout(cs, None, U, x0=parts[m])[0])
    # an ensemble: a member per particle, one value for all
    kw = dict(ds=cs["ds"]) if cs["DS"] == 8 else {}
    nets = [R.make_net(500 + e, cs["dc"], cs["hidden_layers"], cs["activation"], cs["residual"], **kw) for e in range(3)]
    members = [model_of(cs, (), Ws=Ws, bs=bs) for Ws, bs in nets]
    ens = MLPEnsemble(members, nominal=0)
    ens.set_value(val["Ws"], val["bs"], activation=val["activation"], weight=0.75)
    es, _ = build(cs, T, N, None, lam=LAM, model=ens, risk="mean")
    es.set_option("math", 0)
    order = [2, 0, 1]
    es.set_state_particles(torch.from_numpy(parts), members=order)
    es.forward(x0_of(cs).cuda())
    E = es.particle_costs.cpu().numpy()
    U = es._perturbed_action_seqs.cpu().numpy()
    for m, e in enumerate(order):
        same_bits(f"{name}: member {e} from particle {m}", E[m], plain_costs(cs, members[e], parts[m], T, N))
        if "_relu_" in name:
            same_bits(f"{name}: member {e} against the restatement", E[m],
                      VR.rollout(cs, val, U, weight=0.75, x0=parts[m], table=members[e].table)[0])
    assert not np.array_equal(E[0], E[1])


# ------------------------------------------------------------------------------ 5. weight 0, and switching off
@pytest.mark.parametrize("name", ["mlp41_tanh_2l_res", "mlp84_relu_2l_res"])
@pytest.mark.parametrize("N", [100, 4160])
def test_weight_zero_and_switched_off(name, N):
    cs = TR.case(name)
    T = cs["horizons"][-1]
    x0 = x0_of(cs).cuda()
    val = value_for(cs, 1, "tanh")
    # weight 0 without replace_terminal: the bits of the same handle (reference and mask) without a value
    ref = TR.reference(cs, T)
    a, _ = build(cs, T, N, val, ref=ref, angular=cs["angular"], lam=LAM, weight=0.0)
    b, _ = build(cs, T, N, None, ref=ref, angular=cs["angular"], lam=LAM, terminal=False)
    for math in (0, 1):
        for s in (a, b):
            s.reset()
            s.set_option("math", math)
        ra, rb = a.forward(x0), b.forward(x0)
        assert torch.equal(a._costs, b._costs) and torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]), (name, N, math)
    # set_value(None) on a handle that had only a value: the bits of a fresh default handle, rollout and solve
    for math in (0, 1):
        used = ValueRig(cs, T, N, val, math=math, weight=1.5)
        fresh = ValueRig(cs, T, N, None, math=math, terminal=False)
        with_value = used.rollout(3)
        plain = fresh.rollout(3)
        assert not np.array_equal(with_value, plain)
        n = C.c_int(-1)
        used.h.call("mppi_get_mlp_value", None, C.byref(n), None, None, None, None, None)
        assert n.value == VR.n_floats(cs["DS"])
        used.h.call("mppi_set_mlp_value", None, 0, 0, 0, 0.0, 0, None)
        used.h.call("mppi_get_mlp_value", None, C.byref(n), None, None, None, None, None)
        assert n.value == 0
        for (pa, ca), (pb, cb) in zip(used.four_paths(), fresh.four_paths()):
            same_bits(f"{name} N{N} math {math} switched off: {pa}", ca, cb)
        used.close()
        fresh.close()
    # the solver refuses a terminal_cost whose model has no value (any more)
    s, model = build(cs, T, N, val, lam=LAM)
    s.forward(x0)
    model.set_value(None)
    with pytest.raises(ValueError, match="no value"):
        s.forward(x0)


# ------------------------------------------------------------------------------ 6. a critic learned online
def test_update_value_between_two_solves():
    cs = TR.case("mlp42_relu_1l_abs")
    T, N = 7, 100
    first, second = value_for(cs, 1, "relu"), value_for(cs, 5, "relu")
    solver, model = build(cs, T, N, first, lam=LAM, weight=0.75)
    solver.set_option("math", 0)
    x0 = x0_of(cs).cuda()
    solver.forward(x0)
    c1, U1 = solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy()
    same_bits("first critic", c1, VR.rollout(cs, first, U1, weight=0.75)[0])
    model.update_value(second["Ws"], second["bs"])
    solver.forward(x0)
    c2, U2 = solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy()
    same_bits("second critic", c2, VR.rollout(cs, second, U2, weight=0.75)[0])
    assert not np.array_equal(c2, VR.rollout(cs, first, U2, weight=0.75)[0])
    model.set_value_weight(-2.0)
    solver.forward(x0)
    U3 = solver._perturbed_action_seqs.cpu().numpy()
    same_bits("new weight", solver._costs.cpu().numpy(), VR.rollout(cs, second, U3, weight=-2.0)[0])
    # a deep copy continues with the value: its own model, the same costs
    twin = copy.deepcopy(solver)
    assert twin._terminal_fused and twin._cost_owner is not model and twin._terminal_cost.__self__ is twin._cost_owner
    a, b = solver.forward(x0), twin.forward(x0)
    assert torch.equal(solver._costs, twin._costs) and torch.equal(a[0], b[0])


# ------------------------------------------------------------------------------ 7. the generic path means the same
@pytest.mark.parametrize("name,replace", [("mlp41_relu_2l_res", False), ("mlp42_tanh_1l_abs", True), ("mlp82_tanh_2l_res", False),
                                          ("mlp84_relu_2l_res", True)])
def test_generic_path_means_the_same(name, replace):
    cs = TR.case(name)
    T, N = cs["horizons"][-1], 100
    val = value_for(cs, 1, "tanh")
    ref = TR.reference(cs, T)
    x0 = x0_of(cs).cuda()
    eps = torch.from_numpy((np.random.default_rng(9 + T).standard_normal((N, T, cs["dc"])) * f32(cs["sigmas"])).astype(f32))
    outs = []
    for tag in (True, False):
        solver, _ = build(cs, T, N, val, ref=ref, angular=cs["angular"], lam=LAM, tag=tag, weight=1.5, replace=replace)
        assert solver._terminal_fused == tag
        if tag:
            solver.set_option("math", 0)
        solver.inject_noise(eps)
        a, s = solver.forward(x0)
        outs.append((solver._costs.cpu().numpy(), a.cpu().numpy(), s.cpu().numpy()))
    (cn, an, sn), (cg, ag, sg) = outs
    err = rel_err(cg, cn), rel_err(ag, an), rel_err(sg, sn)
    print(f"[mlp-value] {name} replace {replace}: generic against fused: costs {err[0]:.2e}, action {err[1]:.2e}, states {err[2]:.2e} (limit {TOL:g})")
    assert max(err) < TOL, err
    U0 = np.clip(eps.numpy(), f32(cs["u_min"]), f32(cs["u_max"]))
    assert not np.allclose(cn, VR.rollout(cs, None, U0, ref=ref, angular=cs["angular"])[0], rtol=1e-4)


def test_mixed_owners_and_a_model_without_the_keyword():
    """terminal_cost of ANOTHER model next to a tagged pair: the generic path.  A model with a value whose solver was not given
    the keyword: the plain costs, and no value on the handle."""
    cs = TR.case("mlp41_relu_2l_res")
    T, N = 5, 64
    val = value_for(cs, 1, "relu")
    _need_gpu()
    from pi_mpc.mppi import MPPI

    m1, m2 = model_of(cs, ()), model_of(cs, ())
    for m in (m1, m2):
        m.set_value(val["Ws"], val["bs"], activation="relu")
    kw = dict(horizon=T, num_samples=N, dim_state=4, dim_control=1, u_min=torch.tensor(cs["u_min"]), u_max=torch.tensor(cs["u_max"]),
              sigmas=torch.tensor(cs["sigmas"]), lambda_=LAM)
    mixed = MPPI(dynamics=m1.dynamics, cost_func=m1.cost, terminal_cost=m2.terminal_cost, **kw)
    assert mixed._model is None and not mixed._terminal_fused
    plain = MPPI(dynamics=m1.dynamics, cost_func=m1.cost, **kw)
    assert plain._model == "mlp41" and not plain._terminal_fused
    plain.set_option("math", 0)
    plain.forward(x0_of(cs).cuda())
    U = plain._perturbed_action_seqs.cpu().numpy()
    same_bits("no keyword: the plain cost", plain._costs.cpu().numpy(), VR.rollout(cs, None, U)[0])
    n = C.c_int(-1)
    plain._h.call("mppi_get_mlp_value", None, C.byref(n), None, None, None, None, None)
    assert n.value == 0
    with pytest.raises(ValueError):
        MPPI(dynamics=m1.dynamics, cost_func=m1.cost, terminal_cost=3.0, **kw)


# ------------------------------------------------------------------------------ 8. an opaque terminal term on any model
def _nav2d_pair(T, N, known, **kw):
    """(solver with a recording terminal_cost next to nav2d's TAGGED pair, its twin on the generic path without the keyword, seen)"""
    from test_gpu_covariance import _envs

    seen = []

    def terminal(state):
        seen.append(state)
        return known

    solver, x0 = make("nav2d", T, N, LAM, terminal_cost=terminal, **kw)
    env = _envs["nav2d"]
    from pi_mpc.mppi import MPPI

    twin = MPPI(horizon=T, num_samples=N, dim_state=3, dim_control=2, dynamics=lambda s, a: env.dynamics(s, a),
                cost_func=lambda s, a, i: env.cost_function(s, a, i), u_min=solver._u_min.cpu(), u_max=solver._u_max.cpu(),
                sigmas=solver._sigmas.cpu(), lambda_=LAM)
    assert solver._model is None and twin._model is None and solver._recognized is None
    return solver, twin, x0.cuda(), seen


def test_opaque_terminal_cost_on_a_native_pair():
    T, N = 12, 300
    known = torch.from_numpy(np.random.default_rng(4).uniform(-50.0, 50.0, N).astype(f32)).cuda()
    solver, twin, x0, seen = _nav2d_pair(T, N, known)
    a, _ = solver.forward(x0)
    b, _ = twin.forward(x0)
    assert torch.equal(solver._perturbed_action_seqs, twin._perturbed_action_seqs)
    want = twin._costs + known  # float32: one rounding per sample
    assert torch.equal(solver._costs, want) and not torch.equal(solver._costs, twin._costs)
    assert len(seen) == 1 and seen[0].shape == (N, 3) and torch.equal(seen[0], solver._state_seq_batch[:, -1, :])
    assert not torch.equal(a, b)  # (everything downstream sees the sum)
    # three state particles: every row carries it
    solver, twin, x0, seen = _nav2d_pair(T, N, known)
    parts = torch.stack([x0.cpu() + 0.2 * j for j in range(3)])
    for s in (solver, twin):
        s.set_state_particles(parts)
        s.forward(x0)
    E, F = solver.particle_costs, twin.particle_costs
    assert E.shape == (3, N) and len(seen) == 3
    for m in range(3):
        assert torch.equal(E[m], F[m] + known), m


def test_opaque_terminal_cost_in_a_captured_graph():
    """graph_callables=True: warm-up, capture and replay solves equal the eager solver's bit for bit."""
    T, N = 12, 300
    known = torch.from_numpy(np.random.default_rng(5).uniform(-50.0, 50.0, N).astype(f32)).cuda()
    eager, twin, x0, _ = _nav2d_pair(T, N, known)
    graphed, _, _, seen = _nav2d_pair(T, N, known, graph_callables=True)
    states = []
    for tick in range(4):
        a, s = eager.forward(x0)
        b, r = graphed.forward(x0)
        states.append(graphed._graph_state)
        assert torch.equal(eager._costs, graphed._costs) and torch.equal(a, b) and torch.equal(s, r), tick
        if tick == 0:
            twin.forward(x0)
            assert torch.equal(eager._costs, twin._costs + known)
        x0 = s[0, 1].clone()
    assert states[-1] == "replay" and len(seen) == 2  # (called in the warm-up and in the capture, never in a replay)


# ------------------------------------------------------------------------------ 9. the C ABI
def _get_value(h, DS, stream=None):
    n, layers, act, rep, w = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_float(-1.0)
    h.call("mppi_get_mlp_value", None, C.byref(n), C.byref(layers), C.byref(act), C.byref(w), C.byref(rep), stream)
    out = np.full(max(n.value, 1), -7.0, f32)
    if n.value:
        h.call("mppi_get_mlp_value", _vp(out), None, None, None, None, None, stream)
    return out[:n.value], n.value, layers.value, act.value, w.value, rep.value


def test_c_abi_round_trips_and_refusals():
    from mppi_playground_amd import _capi

    cs = TR.case("mlp81_relu_2l_res_s6")
    T, N, DS = 5, 100, 8
    val = value_for(cs, 2, "relu")
    vt = VR.pack(val["Ws"], val["bs"], cs["ds"], DS)
    src, dst = _raw_handle(cs, T, N), _raw_handle(cs, T, N)
    par, tab = np.ascontiguousarray(cs["params"], f32), np.ascontiguousarray(cs["table"], f32)
    x0 = x0_of(cs).cuda()
    # the value BEFORE the weights and the mask: the flags word has one owner
    src.call("mppi_set_mlp_value", _vp(vt), int(vt.size), 2, 0, 0.75, 1, None)
    src.call("mppi_set_mlp_angular", TR.mask(cs["angular"]))
    src.call("mppi_set_model_params", _vp(par), int(par.size))
    src.call("mppi_set_mlp", _vp(tab), int(tab.size), cs["hidden_layers"], 0, int(cs["residual"]), None)
    got = _get_value(src, DS)
    same_bits("read back", got[0], vt)
    assert got[1:] == (vt.size, 2, 0, 0.75, 1)
    mask = C.c_uint32(0)
    src.call("mppi_get_mlp_angular", C.byref(mask))
    assert mask.value == TR.mask(cs["angular"])
    for h in (src, dst):
        h.call("mppi_set_option", b"math", 0)
    src.call("mppi_set_state", x0.data_ptr(), 1, None)
    src.call("mppi_sample", 2, None)
    src.call("mppi_rollout_cost", None)
    dst.call("mppi_clone_state", src.h)
    got = _get_value(dst, DS)
    same_bits("the clone's table", got[0], vt)
    assert got[1:] == (vt.size, 2, 0, 0.75, 1)
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
    same_bits("against the restatement", costs[1],
              VR.rollout(cs, val, U.cpu().numpy(), angular=cs["angular"], weight=0.75, replace_terminal=True)[0])
    # a clone of a handle without a value clears the destination's
    bare = _raw_handle(cs, T, N)
    dst.call("mppi_clone_state", bare.h)
    assert _get_value(dst, DS)[1] == 0
    # refusals
    with pytest.raises(_capi.MppiError, match=r"\(-1\).*wrong number"):
        src.call("mppi_set_mlp_value", _vp(vt), int(vt.size) - 1, 2, 0, 1.0, 0, None)
    bad = vt.copy()
    for v in (np.nan, np.inf):
        bad[17] = v
        with pytest.raises(_capi.MppiError, match=r"\(-1\).*finite"):
            src.call("mppi_set_mlp_value", _vp(bad), int(bad.size), 2, 0, 1.0, 0, None)
    for layers, act, w, rep in ((3, 0, 1.0, 0), (0, 0, 1.0, 0), (2, 7, 1.0, 0), (2, 0, float("nan"), 0), (2, 0, float("inf"), 0), (2, 0, 1.0, 2)):
        with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
            src.call("mppi_set_mlp_value", _vp(vt), int(vt.size), layers, act, w, rep, None)
    assert _get_value(src, DS)[1:] == (vt.size, 2, 0, 0.75, 1)  # (a refused call changes nothing)
    pend, _ = make("pendulum", 8, 64, 1.0)
    n = C.c_int(0)
    for call in (lambda: pend._h.call("mppi_set_mlp_value", _vp(vt), int(vt.size), 2, 0, 1.0, 0, None),
                 lambda: pend._h.call("mppi_set_mlp_value", None, 0, 0, 0, 0.0, 0, None),
                 lambda: pend._h.call("mppi_get_mlp_value", None, C.byref(n), None, None, None, None, None)):
        with pytest.raises(_capi.MppiError, match=r"\(-1\)"):
            call()
    for h in (src, dst, bare):
        h.close()


def test_state_dict_round_trip_keeps_the_value():
    cs = TR.case("mlp42_relu_1l_abs")
    T, N = 7, 100
    val = value_for(cs, 1, "relu")
    model = model_of(cs, ())
    a, _ = build(cs, T, N, val, lam=LAM, model=model, weight=0.75, replace=True)
    x0 = x0_of(cs).cuda()
    for s in (a,):
        s.set_option("math", 0)
        s.forward(x0)
    b, _ = build(cs, T, N, None, lam=LAM, model=model)
    b.set_option("math", 0)
    b.load_state_dict(a.state_dict())
    ra, rb = a.forward(x0), b.forward(x0)
    assert torch.equal(a._costs, b._costs) and torch.equal(ra[0], rb[0])
    got = _get_value(b._h, 4, b._stream())
    same_bits("the table on the second handle", got[0], VR.pack(val["Ws"], val["bs"], cs["ds"], 4))
    assert got[1:] == (VR.n_floats(4), val["hidden_layers"], 0, 0.75, 1)
    U = b._perturbed_action_seqs.cpu().numpy()
    same_bits("against the restatement", b._costs.cpu().numpy(), VR.rollout(cs, val, U, weight=0.75, replace_terminal=True)[0])
