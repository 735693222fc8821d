"""The control-cost term (action_cost=True; src/pi_mpc/mppi.py:294-316,330-336) on a real MI355X.

The basic measurement (`measure`): ONE handle with the term enabled rolls out the same solve index twice around the same
non-zero mean, at weight 0 and at weight 1 — the same instantiation and the same noise, so c(0) is the stage + terminal cost c0
bit for bit — and exports U.  Then, for EVERY sample (tests/action_cost_ref.py: check),
  (a) c(1) == fl32(c(0) + fl32(kappa * A32)) bit for bit, A32 the numpy fp32 restatement of the sequential sum, and
  (b) |c(1) - (c(0) + kappa * A64)| <= 2 * 2^-24 * (|c(1)| + (T * dc + 1) * kappa * sum |g * U|): the first-order bound of a
      sequential fp32 sum of T * dc products plus two roundings, doubled.
The shapes are the smallest that reach each copy of the horizon loop.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import action_cost_ref as ref
from helpers import MODEL_CFG, orc, rel_err
from test_gpu_covariance import _need_gpu, make, weights64
from test_gpu_fused_geometry import Raw, took

pytestmark = pytest.mark.gpu

f32 = np.float32
LAM = 3.0  # the temperature of the raw-handle cases: kappa = 3 keeps the term of the order of the costs


def make_any(model, T, N, lam, **kw):
    """test_gpu_covariance.make, plus the three shipped models it does not build."""
    if model in ("pendulum", "cartpole", "nav2d", "racing"):
        return make(model, T, N, lam, **kw)
    _need_gpu()
    from pi_mpc.mppi import MPPI

    cfg = MODEL_CFG[model]
    common = dict(horizon=T, num_samples=N, u_min=torch.tensor(cfg["u_min"]), u_max=torch.tensor(cfg["u_max"]),
                  sigmas=torch.tensor(cfg["sigmas"]), lambda_=lam, **kw)
    if model == "goalzone":
        from envs.goal_in_danger_zone import GoalInDangerZoneEnv
        from helpers import goalzone_env_fixture

        env = GoalInDangerZoneEnv()
        env._goal = goalzone_env_fixture()["goal"]
        solver = MPPI(dim_state=7, dim_control=2, dynamics=env.parallel_step, cost_func=env.parallel_cost, **common)
        solver._test_keep = env
        return solver, torch.from_numpy(np.asarray(goalzone_env_fixture()["x0"], f32))
    from envs import classic_control as cc

    ds, dc = orc.MODEL_DIMS[orc.MODEL_IDS[model]]
    x0 = {"mountaincar": [-0.5, 0.0], "mjcartpole": [0.0, 0.0, 0.05, 0.0]}[model]
    return (MPPI(dim_state=ds, dim_control=dc, dynamics=getattr(cc, f"{model}_dynamics"), cost_func=getattr(cc, f"{model}_cost"),
                 **common), torch.tensor(x0))


class Rig(Raw):
    """test_gpu_fused_geometry.Raw (a native handle driven through the C ABI) around any shipped model and any solver keyword."""

    def __init__(self, model, T, N, x0=None, solver=None, **kw):
        self.model, self.T, self.N = model, T, N
        if solver is None:
            solver, x = make_any(model, T, N, 1.0, **kw)
        else:
            solver, x = solver
        self.solver = solver
        x0 = x if x0 is None else torch.as_tensor(np.asarray(x0, f32))
        self.dc, self.ds = solver._dim_control, solver._dim_state
        self.x0 = x0.to("cuda", torch.float32).contiguous()
        self.action = torch.empty(T, self.dc, device="cuda")
        self.state = torch.empty(1, T + 1, self.ds, device="cuda")
        self.stats = torch.empty(4, device="cuda")
        self.mode = None
        self._prepare()


def term(rig, weight, lam=LAM):
    rig.h.call("mppi_set_action_cost", 1, float(weight))
    rig.h.call("mppi_set_action_cost_lambda", float(lam))


def random_mean(rig, seed):
    """Uniform inside the control bounds, [T, dc]."""
    cfg = MODEL_CFG[rig.model]
    rng = np.random.default_rng(seed)
    return rng.uniform(f32(cfg["u_min"]), f32(cfg["u_max"]), (rig.T, rig.dc)).astype(f32)


def sigmas_of(rig):
    return rig.solver._sigmas.cpu().numpy()


def measure(name, rig, idx=3, mean=None, lam=LAM, sig=None):
    """-> (c0, c1, U, g): the two rollouts of solve `idx` on one handle, both checks on every sample."""
    mean = random_mean(rig, idx) if mean is None else np.asarray(mean, f32)
    rig.set_mean(mean)
    term(rig, 0.0, lam)
    c0 = rig.rollout(idx)
    term(rig, 1.0, lam)
    c1 = rig.rollout(idx)
    U = rig.actions_around(mean)
    g = ref.g32(mean, sigmas_of(rig) if sig is None else sig)
    assert np.all(np.isfinite(c0)) and np.all(np.isfinite(c1)), name
    ref.check(name, c1, c0, ref.kappa32(1.0, lam), g, U)
    return c0, c1, U, g


# ------------------------------------------------------------------------------ 1. row shapes
ROWS = ([("pendulum", T) for T in (1, 2, 5, 15, 16)] + [("nav2d", 30), ("racing", 25), ("racing", 26), ("cartpole", 8),
        ("mountaincar", 8), ("mjcartpole", 6), ("goalzone", 6)])


@pytest.mark.parametrize("N", [65, 200])
@pytest.mark.parametrize("model,T", ROWS)
def test_row_shapes(model, T, N):
    rig = Rig(model, T, N)
    c0, c1, U, g = measure(f"{model}_T{T}_N{N}", rig)
    if T == 1:  # row 0 of the inverse covariance is zero: the term is identically 0
        assert np.array_equal(c1.view(np.uint32), c0.view(np.uint32))
    else:
        assert np.any(c1 != c0)
    rig.close()


# ------------------------------------------------------------------------------ 2. every math level
@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("model,T", [("pendulum", 15), ("nav2d", 30), ("racing", 25)])
def test_math_levels(model, T, math):
    rig = Rig(model, T, 200)
    rig.h.call("mppi_set_option", b"math", math)
    measure(f"{model}_math{math}", rig)
    rig.close()


# ------------------------------------------------------------------------------ 3. regenerated noise and tiles
@pytest.mark.parametrize("model,T", [("pendulum", 15), ("pendulum", 16), ("nav2d", 30), ("racing", 25), ("racing", 26)])
def test_regenerated_noise_equals_tiles(model, T):
    rig = Rig(model, T, 200)
    _, c1, _, _ = measure(f"{model}_T{T}_regen", rig)
    rig.h.call("mppi_set_option", b"noise_regen", 0)
    _, c1t, _, _ = measure(f"{model}_T{T}_tiles", rig)
    assert np.array_equal(c1.view(np.uint32), c1t.view(np.uint32))
    rig.close()


# ------------------------------------------------------------------------------ 4. the launch-uniform copies
def _racing_with_wheel_base(L, T, N):
    _need_gpu()
    from envs.racing_controller import racing_controller
    from envs.racing_env import RacingEnv

    env = RacingEnv()
    env.L = torch.tensor(L, device=env.L.device, dtype=env.L.dtype)
    ctrl = racing_controller(env, horizon=T, num_samples=N, lambda_=1.0)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    r, _ = ctrl.calc_ref_trajectory(env._robot_state, env.racing_center_path, 0, T, DL=0.1, lookahead_distance=3,
                                    reference_path_interval=0.85)
    ctrl.set_reference(r)
    ctrl.solver._test_keep = ctrl
    return ctrl.solver, env._robot_state.clone()


@pytest.mark.parametrize("L", [1.0, 1.3])
def test_racing_wheel_base(L):
    rig = Rig("racing", 25, 200, solver=_racing_with_wheel_base(L, 25, 200))
    measure(f"racing_L{L}", rig)
    rig.close()


@pytest.mark.parametrize("model,T,x0", [("nav2d", 30, [-40.0, -9.0, 0.785]), ("racing", 25, None)])
def test_start_outside_the_position_clamp(model, T, x0):
    """x0 beyond the map's edge: the copy of the loop whose first stage cost takes the bounds-tested lookup."""
    if x0 is None:
        _, s = make("racing", T, 64, 1.0)
        x0 = s.detach().cpu().numpy().copy()
        x0[0] = 41.5  # (the map spans +-40 m)
    rig = Rig(model, T, 200, x0=x0)
    inside = Rig(model, T, 200)
    c0, _, _, _ = measure(f"{model}_x0_outside", rig)
    ci, _, _, _ = measure(f"{model}_x0_inside", inside)
    assert not np.array_equal(c0, ci)
    rig.close()
    inside.close()


def test_pendulum_lane_through_the_library_math_redo():
    """A start that sends lanes out of the fast path's range (picked with the host build of the functors): the redo carries
    the term too."""
    import emul

    T, N = 15, 200
    rig = Rig("pendulum", T, N)
    mean = random_mean(rig, 3)
    rig.set_mean(mean)
    st = rig.solver._stream()
    rig.h.call("mppi_sample", 3, st)
    eps = torch.empty(N, T, 1, device="cuda")
    rig.h.call("mppi_export_noise", eps.data_ptr(), None, st)
    eps = eps.cpu().numpy()
    cfg = MODEL_CFG["pendulum"]
    picked = None
    for x0 in ([150.0, -3.0], [-199.0, 8.0], [250.0, 1.0], [-9.9e4, 7.9], [1.2e5, -8.0], [0.0, 100.0]):
        _, bad, _ = emul.rollout_cost(orc.MODEL_IDS["pendulum"], 1, f32(x0), mean, eps, cfg["u_min"], cfg["u_max"], N)
        if bad.any():
            picked = (x0, int(bad.sum()))
            break
    assert picked is not None, "no candidate start leaves the pendulum's fast path on the host build"
    rig.close()
    rig = Rig("pendulum", T, N, x0=picked[0])
    print(f"[action_cost] pendulum redo: x0 {picked[0]}, {picked[1]} of {N} lanes redo on the host build")
    measure("pendulum_redo", rig)
    rig.close()


# ------------------------------------------------------------------------------ 5. exploration, 6. saturation, 7. zero mean
@pytest.mark.parametrize("model,T", [("pendulum", 15), ("nav2d", 30)])
def test_exploration_threshold_inside_a_tile(model, T):
    """N = 200, exploration 0.3: samples 140.. do not inherit the mean when sampling, and still get g from the real mean."""
    rig = Rig(model, T, 200, exploration=0.3)
    assert rig.solver._h is not None and int(200 * (1 - 0.3)) == 140
    c0, c1, U, g = measure(f"{model}_explore", rig)
    assert np.any((c1 != c0)[140:]), "the exploration samples carry the term"
    # (their exported rows are clamp(0 + eps): around the mean's own rows the handle without exploration holds other actions)
    plain = Rig(model, T, 200)
    plain.h.call("mppi_sample", 3, plain.solver._stream())
    Up = plain.actions_around(rig._mean.cpu().numpy())
    assert np.array_equal(Up[:140], U[:140]) and not np.array_equal(Up[140:], U[140:])
    plain.close()
    rig.close()


@pytest.mark.parametrize("model,T,sig", [("pendulum", 15, [12.0]), ("nav2d", 30, [6.0, 6.0])])
def test_saturated_actions(model, T, sig):
    """sigmas = 3 x (u_max - u_min): most of U on a bound."""
    rig = Rig(model, T, 200, sigmas=sig)
    _, _, U, _ = measure(f"{model}_saturated", rig)
    cfg = MODEL_CFG[model]
    assert np.mean((U == f32(cfg["u_min"])) | (U == f32(cfg["u_max"]))) > 0.5
    rig.close()


def test_zero_mean_changes_nothing():
    for model, T in (("pendulum", 15), ("racing", 25)):
        rig = Rig(model, T, 200)
        c0, c1, _, _ = measure(f"{model}_zero_mean", rig, mean=np.zeros((T, rig.dc), f32))
        assert np.array_equal(c1.view(np.uint32), c0.view(np.uint32))
        rig.close()
    # ... and the first forward() of a fresh solver: zero warm start, whatever the weight
    outs = []
    for w in (0.0, 1.0):
        solver, x0 = make("pendulum", 15, 1000, 20.0, action_cost=True, action_cost_weight=w)
        a, s = solver.forward(x0.cuda())
        outs.append((solver._costs.clone(), a.clone(), s.clone()))
    for p, q in zip(*outs):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------ 8. window handles
@pytest.mark.parametrize("inherit", [None, 160])
def test_window_handles_equal_the_unsharded_handle(inherit):
    """Samples [0, 130) and [130, 200) on handles of their own (as the shards of a sharded solver hold them), the term
    re-enabled on each re-created handle; with the exploration threshold (160) inside the second window."""
    T, N = 15, 200
    whole = Rig("pendulum", T, N, **({} if inherit is None else dict(exploration=0.2)))
    if inherit is not None:
        assert whole.solver._h is not None and int(N * (1 - 0.2)) == inherit
    mean = random_mean(whole, 5)
    _, c1, _, _ = measure("window_whole", whole, idx=5, mean=mean)
    parts = []
    for off, n in ((0, 130), (130, 70)):
        w = Raw("pendulum", T, n, offset=off, inherit=(1 << 40) if inherit is None else inherit)
        _, cw, _, _ = measure(f"window_{off}_{n}", w, idx=5, mean=mean)
        parts.append(cw)
        w.close()
    got = np.concatenate(parts)
    assert np.array_equal(got.view(np.uint32), c1.view(np.uint32))
    whole.close()


# ------------------------------------------------------------------------------ 9. the separate pass on a native handle
@pytest.mark.parametrize("model,T,kw", [("pendulum", 15, {}), ("racing", 25, {}), ("nav2d", 30, dict(exploration=0.3))])
def test_separate_pass_equals_the_rollout(model, T, kw):
    rig = Rig(model, T, 200, **kw)
    mean = random_mean(rig, 7)
    c0, c1, U, g = measure(f"{model}_in_rollout", rig, idx=7, mean=mean)
    term(rig, 0.0)
    assert np.array_equal(rig.rollout(7), c0)
    term(rig, 1.0)
    st = rig.solver._stream()
    rig.h.call("mppi_add_action_cost", LAM, st)
    added = rig.costs()
    ref.check(f"{model}_separate_pass", added, c0, ref.kappa32(1.0, LAM), g, U)
    assert np.array_equal(added.view(np.uint32), c1.view(np.uint32))
    rig.close()


# ------------------------------------------------------------------------------ 10. generic handles
def _callables(dc):
    B = torch.linspace(-0.1, 0.1, 2 * dc, device="cuda").reshape(2, dc)

    def dynamics(state, action):
        return state + action @ B.T

    def cost(state, action, info):
        return (state ** 2).sum(dim=1) + 0.05 * (action ** 2).sum(dim=1)

    return dynamics, cost


GENERIC = {3: dict(u_min=[-1.0, -0.5, -2.0], u_max=[0.5, 0.6, 1.0], sigmas=[0.5, 1.0, 2.0]),
           6: dict(u_min=[-1.0, -0.5, -2.0, -0.3, -1.5, -0.7], u_max=[0.5, 0.6, 1.0, 0.9, 0.2, 0.7],
                   sigmas=[0.5, 1.0, 2.0, 0.25, 0.75, 1.5])}


def _generic(dc, T, N, **kw):
    _need_gpu()
    from pi_mpc.mppi import MPPI

    dyn, cost = _callables(dc)
    lim = GENERIC[dc]
    return MPPI(horizon=T, num_samples=N, dim_state=2, dim_control=dc, dynamics=dyn, cost_func=cost,
                u_min=torch.tensor(lim["u_min"]), u_max=torch.tensor(lim["u_max"]), sigmas=torch.tensor(lim["sigmas"]),
                lambda_=2.0, exploration=0.1, **kw)


@pytest.mark.parametrize("dc,T", [(3, 45), (6, 7)])
def test_separate_pass_on_generic_handles(dc, T):
    """Wide rows (the control index of a column depends on its float4 group; per-column sigmas and bounds), costs injected."""
    N = 384
    solver = _generic(dc, T, N, action_cost=True)
    assert solver._model is None
    h, st = solver._h, solver._stream()
    rng = np.random.default_rng(dc)
    lim = GENERIC[dc]
    mean = rng.uniform(f32(lim["u_min"]), f32(lim["u_max"]), (T, dc)).astype(f32)
    m = torch.from_numpy(mean).cuda()
    h.call("mppi_set_mean", m.data_ptr(), 1, st)
    h.call("mppi_sample", 9, st)
    c0 = (rng.standard_normal(N) * 30.0 + 50.0).astype(f32)
    c = torch.from_numpy(c0).cuda()
    h.call("mppi_set_costs", c.data_ptr(), 1, st)
    h.call("mppi_add_action_cost", LAM, st)
    c1 = solver._costs.cpu().numpy()
    U = torch.empty(N, T, dc, device="cuda")
    h.call("mppi_export_noise", None, U.data_ptr(), st)
    U = U.cpu().numpy()
    ref.check(f"generic_dc{dc}", c1, c0, ref.kappa32(1.0, LAM), ref.g32(mean, f32(lim["sigmas"])), U)
    # the minimum key is the minimum of the NEW costs: a softmax statistics pass reports it
    stats = (C.c_double * 8)()
    h.call("mppi_softmax_stats", 2.0, stats, st)
    assert f32(stats[0]) == c1.min() and c1.min() != c0.min()


# ------------------------------------------------------------------------------ whole solves through MPPI
def shadow_costs(shadow, x, idx, mean, sigma_seq=None):
    """c0 of a tick: the shadow solver (same configuration and seed, weight 0) rolls solve `idx` out around `mean` from `x`."""
    h, st = shadow._h, shadow._stream()
    shadow._refresh_model_inputs()
    x = x.detach().to("cuda", torch.float32).contiguous()
    m = torch.from_numpy(np.ascontiguousarray(mean, f32)).cuda()
    h.call("mppi_set_state", x.data_ptr(), 1, st)
    h.call("mppi_set_mean", m.data_ptr(), 1, st)
    if sigma_seq is not None:
        h.call("mppi_set_sigma_table", sigma_seq.data_ptr(), 1, st)
    h.call("mppi_set_action_cost_lambda", 1.0)
    h.call("mppi_sample", idx, st)
    h.call("mppi_rollout_cost", st)
    return shadow._costs.cpu().numpy()


def current_mean(solver):
    m = torch.empty(solver._horizon, solver._dim_control, device="cuda")
    solver._h.call("mppi_get_mean", m.data_ptr(), 1, solver._stream())
    return m.cpu().numpy()


def softmax_action(costs, lam, U):
    e, _ = weights64(costs, lam)
    return ((e / e.sum())[:, None, None] * np.asarray(U, np.float64)).sum(0)


def closed_loop(name, solver, shadow, x0, ticks, lam_of, sg=False, table=False, warm=None):
    """`ticks` closed-loop forward() calls; every tick's costs against the shadow's c0 (checks (a) and (b)) and its action_seq
    against the float64 softmax over the device's own costs and exported U.  lam_of(tick, solver, previous) -> (temperature
    of the term, temperature of the weights)."""
    from pi_mpc import _host

    x = x0.cuda()
    if warm is not None:
        solver.set_warm_start(warm)
    prev_lam = None
    for tick in range(ticks):
        mean, idx = current_mean(solver), solver._solve_idx
        sig = solver.sigma_seq.clone() if table else None
        hist = np.array(solver._actions_history_for_sg, copy=True) if sg else None
        a, s = solver.forward(x)
        assert took(solver._h) == (0, 0), "the term lives on the multi-kernel path"
        c1 = solver._costs.cpu().numpy()
        U = solver._perturbed_action_seqs.cpu().numpy()
        lam_term, lam_w = lam_of(tick, solver, prev_lam)
        prev_lam = float(solver._last_lambda)
        c0 = shadow_costs(shadow, x, idx, mean, sig)
        g = ref.g32(mean, solver._sigmas.cpu().numpy() if sig is None else sig.cpu().numpy())
        ref.check(f"{name}_tick{tick}", c1, c0, ref.kappa32(solver._action_cost_weight, lam_term), g, U)
        if tick > 0 or warm is not None:
            assert np.any(mean != 0.0)
        want = softmax_action(c1, lam_w, U)
        if sg:
            want = _host.sg_filter_sequence(hist, want, solver._coeffs)
        err = rel_err(a.cpu().numpy(), want)
        print(f"[action_cost] {name} tick {tick}: action_seq rel err {err:.3e}, lambda term {lam_term:.6g} weights {lam_w:.6g}")
        assert err < 1e-5, (name, tick, err)
        x = s[0, 1].clone()


@pytest.mark.parametrize("model,T,N,lam,kw", [("pendulum", 15, 1000, 20.0, {}), ("racing", 25, 512, 50.0, {}),
                                              ("nav2d", 30, 1024, 100.0, dict(use_sg_filter=True))])
def test_closed_loop_fixed_temperature(model, T, N, lam, kw):
    solver, x0 = make(model, T, N, lam, action_cost=True, **kw)
    shadow, _ = make(model, T, N, lam, action_cost=True, action_cost_weight=0.0, **kw)
    closed_loop(f"{model}_fixed", solver, shadow, x0, 3, lambda tick, s, prev: (lam, lam), sg=bool(kw))


@pytest.mark.parametrize("rule", ["MPO", "ESSPS"])
def test_closed_loop_device_temperature(rule):
    """kappa = fl32(weight * lambda) with the temperature in device memory when the rollout starts: MPO — the dual's current
    one, which is also the one this tick's weights use; ESSPS — the previous tick's result, 0 on the first tick (the warm start
    is set by hand here so that a wrong factor would show)."""
    T, N = 15, 1000
    kw = dict(essps_target_ess=100.0, lambda_min=1e-3, lambda_max=1e5) if rule == "ESSPS" else {}
    solver, x0 = make("pendulum", T, N, rule, action_cost=True, **kw)
    shadow, _ = make("pendulum", T, N, 1.0, action_cost=True, action_cost_weight=0.0)
    assert solver._rule_on_device == rule

    def lam_of(tick, s, prev):
        used = float(s._last_lambda)
        if rule == "MPO":
            return used, used
        return (0.0 if prev is None else prev), used

    warm = np.random.default_rng(1).uniform(-1.0, 1.0, (T, 1)).astype(f32)
    closed_loop(f"pendulum_{rule}", solver, shadow, x0, 3, lam_of, warm=warm)


def test_closed_loop_with_adapted_covariance():
    """adapt_covariance: g follows `sigma_seq` as read before each tick (the shadow draws from the same table)."""
    T, N, lam = 30, 1024, 100.0
    kw = dict(adapt_covariance=True, cov_rate=0.5, sigma_min=torch.tensor([0.05, 0.05]))
    solver, x0 = make("nav2d", T, N, lam, action_cost=True, **kw)
    shadow, _ = make("nav2d", T, N, lam, action_cost=True, action_cost_weight=0.0, **kw)
    closed_loop("nav2d_adapted", solver, shadow, x0, 3, lambda tick, s, prev: (lam, lam), table=True)
    assert not torch.equal(solver.sigma_seq, solver._sigmas.repeat(T, 1))


def test_generic_path_end_to_end():
    """Opaque callables at dim_control = 3: the term arrives through mppi_add_action_cost after the callables' costs, outside
    the captured graph — plain and graph_callables=True bit-identical, and the costs held to both checks."""
    T, N, dc = 45, 384, 3
    x0 = torch.tensor([1.0, -0.5])
    outs = []
    for graph in (False, True):
        solver = _generic(dc, T, N, action_cost=True, graph_callables=graph)
        rec = []
        for tick in range(4):
            mean = current_mean(solver)
            a, s = solver.forward(x0)
            c1 = solver._costs.cpu().numpy()
            rec += [a.clone(), torch.as_tensor(s).clone(), solver._costs.clone()]
            if not graph:
                c0 = solver._generic_costs_keep.detach().cpu().numpy().astype(f32)
                U = solver._perturbed_action_seqs.cpu().numpy()
                ref.check(f"generic_e2e_tick{tick}", c1, c0, ref.kappa32(1.0, 2.0), ref.g32(mean, f32(GENERIC[dc]["sigmas"])), U)
                if tick:
                    assert np.any(c1 != c0)
        if graph:
            assert solver._graph_state == "replay"
        outs.append(rec)
    for p, q in zip(*outs):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------ 15. protocol and guards
def _loop(solver, x, n):
    out = []
    for _ in range(n):
        a, s = solver.forward(x)
        out += [a.clone(), s.clone(), solver._costs.clone()]
        x = s[0, 1].clone()
    return out, x


def test_deepcopy_and_state_dict_continue_bit_identically():
    T, N = 15, 512
    kw = dict(action_cost=True, action_cost_weight=0.5)
    a, x0 = make("pendulum", T, N, 20.0, **kw)
    _, xa = _loop(a, x0.cuda(), 2)
    c = copy.deepcopy(a)
    d, _ = make("pendulum", T, N, 20.0, **kw)
    d.load_state_dict(a.state_dict())
    assert c._action_cost and c._action_cost_weight == 0.5
    ra, _ = _loop(a, xa, 2)
    for other in (c, d):
        ro, _ = _loop(other, xa, 2)
        for p, q in zip(ra, ro):
            assert torch.equal(p, q)
    # ... and the term is really on in all of them: a solver without it has other costs from the same state
    e, _ = make("pendulum", T, N, 20.0)
    e.load_state_dict(c.state_dict())
    c2, _ = _loop(c, xa, 1)
    e2, _ = _loop(e, xa, 1)
    assert not torch.equal(c2[2], e2[2])


def test_guards():
    from mppi_playground_amd import _capi

    solver, x0 = make("pendulum", 15, 256, 1.0, action_cost=True)
    with pytest.raises(_capi.MppiError):
        solver.set_option("mapping", 1)
    plain, _ = make("pendulum", 15, 256, 1.0)
    plain.set_option("mapping", 1)
    with pytest.raises(_capi.MppiError):
        plain._h.call("mppi_set_action_cost", 1, 1.0)
    with pytest.raises(_capi.MppiError):
        solver._h.call("mppi_set_action_cost", 1, -1.0)
    with pytest.raises(ValueError):
        make("pendulum", 15, 256, 1.0, action_cost=True, action_cost_weight=-0.5)
    with pytest.raises(ValueError):
        make("pendulum", 15, 256, 1.0, action_cost=True, sigmas=[0.0])
    with pytest.raises(ValueError):
        make("nav2d", 30, 256, 1.0, action_cost=True, adapt_covariance=True, cov_floor=0.0)


def test_single_launch_only_without_the_term():
    N = 4000
    on, x0 = make("pendulum", 15, N, 1.0, action_cost=True)
    off, _ = make("pendulum", 15, N, 1.0)
    on.forward(x0.cuda())
    off.forward(x0.cuda())
    assert took(on._h) == (0, 0)
    g, spb = took(off._h)
    assert g > 0 and spb > 0


@pytest.mark.parametrize("model,T,N,lam", [("pendulum", 15, 1000, 20.0), ("racing", 25, 512, 50.0)])
def test_default_solver_is_unchanged(model, T, N, lam):
    """A default solver and an action_cost=False solver: bit-identical over three ticks."""
    outs = []
    for kw in ({}, dict(action_cost=False, action_cost_weight=0.25)):
        solver, x0 = make(model, T, N, lam, **kw)
        rec, _ = _loop(solver, x0.cuda(), 3)
        outs.append(rec)
    for p, q in zip(*outs):
        assert torch.equal(p, q)
