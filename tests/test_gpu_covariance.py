"""Covariance adaptation (adapt_covariance=True, the sketch at src/pi_mpc/mppi.py:400-418) on a real MI355X.

The yardstick for the per-step table is a numpy restatement written here: the solve's clamped actions U[N,T,dc] and costs
come from the device, the weight ARGUMENT is formed in fp32 exactly as the kernels form it,
fl32(fl32((-c)/lambda) - fl32((-c_min)/lambda)) — which keeps the |c|/lambda amplification of the last cost bit (DESIGN.md
section 4) out of the comparison — and everything after it (exp, weighted mean, variance, update rule) is float64.
Limit: 1e-5 relative on every s[t,k]; a case that misses it is held to twice the spread of equally valid fp32 evaluations of
the same sums instead (sequential, reversed, pairwise; computed here), never more.
"""
import copy

import numpy as np
import pytest
import torch

from helpers import MODEL_CFG, orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
f32 = np.float32
_envs = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def make(model, T, N, lambda_, sigmas=None, **kw):
    """(solver, start state) for a shipped native model."""
    _need_gpu()
    from pi_mpc.mppi import MPPI

    cfg = MODEL_CFG[model]
    sig = torch.tensor(cfg["sigmas"] if sigmas is None else sigmas)
    if model == "racing":
        from envs.racing_controller import racing_controller
        from envs.racing_env import RacingEnv

        env = _envs.setdefault("racing", RacingEnv())
        assert sigmas is None
        ctrl = racing_controller(env, horizon=T, num_samples=N, lambda_=lambda_, **kw)
        ctrl.set_cost_map(env._obstacle_map, env._lane_map)
        ref, _ = ctrl.calc_ref_trajectory(env._robot_state, env.racing_center_path, 0, T, DL=0.1, lookahead_distance=3,
                                          reference_path_interval=0.85)
        ctrl.set_reference(ref)
        ctrl.solver._test_keep = ctrl
        return ctrl.solver, env._robot_state.clone()
    common = dict(horizon=T, num_samples=N, u_min=torch.tensor(cfg["u_min"]), u_max=torch.tensor(cfg["u_max"]), sigmas=sig,
                  lambda_=lambda_, **kw)
    if model == "nav2d":
        from envs.navigation_2d import Navigation2DEnv

        env = _envs.setdefault("nav2d", Navigation2DEnv())
        return (MPPI(dim_state=3, dim_control=2, dynamics=env.dynamics, cost_func=env.cost_function, **common),
                torch.tensor([-9.0, -9.0, 0.785]))
    from envs import classic_control as cc

    ds, dc = orc.MODEL_DIMS[orc.MODEL_IDS[model]]
    x0 = {"pendulum": [3.0, 0.1], "cartpole": [0.01, 0.0, 0.02, 0.0]}[model]
    return (MPPI(dim_state=ds, dim_control=dc, dynamics=getattr(cc, f"{model}_dynamics"), cost_func=getattr(cc, f"{model}_cost"),
                 **common), torch.tensor(x0))


# ------------------------------------------------------------------------------ the restatement
def weights64(costs, lam):
    """(e, ESS): un-normalised weights from the fp32 argument the kernels form, exp and everything after in float64."""
    c, lam = np.asarray(costs, f32), f32(lam)
    arg = ((-c) / lam).astype(f32) - f32((-c.min()) / lam)
    e = np.exp(arg.astype(f32).astype(np.float64))
    return e, float(e.sum() ** 2 / (e * e).sum())


def restate(U, costs, lam, s_old, rate=1.0, floor=1e-6, smin=0.0, smax=np.inf):
    """s[T,dc] after the step, float64: var = sum w (U - ubar)^2 with ubar the weighted mean (no filter), then the rule."""
    e, _ = weights64(costs, lam)
    U = np.asarray(U, np.float64)
    w = (e / e.sum())[:, None, None]
    ubar = (w * U).sum(0)
    var = (w * (U - ubar) ** 2).sum(0)
    s2 = (1.0 - rate) * np.asarray(s_old, np.float64) ** 2 + rate * (var + floor)
    return np.clip(np.sqrt(s2), smin, smax), var


def fp32_spread(U, costs, lam, s_old, s64, rate=1.0, floor=1e-6, smin=0.0, smax=np.inf):
    """Largest relative distance on s between the float64 value and three equally valid fp32 evaluations of the same sums
    (sequential, reversed, numpy's pairwise)."""
    e, _ = weights64(costs, lam)
    e32, U32 = e.astype(f32), np.asarray(U, f32)
    worst = 0.0
    for order in ("seq", "rev", "pair"):
        def total(x):
            x = x if order != "rev" else x[::-1]
            return np.sum(x, axis=0, dtype=f32) if order == "pair" else np.cumsum(x, axis=0, dtype=f32)[-1]
        se = total(e32)
        ubar = (total(e32[:, None, None] * U32) / se).astype(f32)
        var = (total((e32[:, None, None] * ((U32 - ubar) ** 2).astype(f32)).astype(f32)) / se).astype(f32)
        s2 = (f32(1.0 - rate) * np.asarray(s_old, f32) ** 2 + f32(rate) * (var + f32(floor))).astype(f32)
        s = np.clip(np.sqrt(s2), smin, smax)
        worst = max(worst, float(np.max(np.abs(s.astype(np.float64) - s64) / s64)))
    return worst


def check_table(name, got, U, costs, lam, s_old, **rule):
    want, var = restate(U, costs, lam, s_old, **rule)
    err = float(np.max(np.abs(np.asarray(got, np.float64) - want) / want))
    _, ess = weights64(costs, lam)
    limit = TOL
    if err > TOL:
        limit = max(TOL, 2.0 * fp32_spread(U, costs, lam, s_old, want, **rule))
    print(f"[covariance] {name}: max rel err of s {err:.3e} (limit {limit:.3e}), ESS {ess:.1f} of {len(costs)}, "
          f"s in [{want.min():.4g}, {want.max():.4g}]")
    assert np.all(np.isfinite(got))
    assert err <= limit, f"{name}: s off by {err:.3e} > {limit:.3e}"
    return want


def solve_and_check(name, solver, x0, lam=None, **rule):
    """One forward(); the table after it against the restatement from that solve's own U, costs and temperature."""
    s_old = solver.sigma_seq.cpu().numpy()
    solver.forward(x0)
    U = solver._perturbed_action_seqs.cpu().numpy()
    costs = solver._costs.cpu().numpy()
    lam = float(solver._last_lambda) if lam is None else lam
    return check_table(name, solver.sigma_seq.cpu().numpy(), U, costs, lam, s_old, **rule)


# ------------------------------------------------------------------------------ 1. the table after one solve
def _ESS(target):
    """Temperature by ESSPS, so that `target` samples carry the weight whatever the model's cost scale is."""
    return dict(essps_target_ess=target, lambda_min=1e-3, lambda_max=1e5)


@pytest.mark.parametrize("name,model,T,N,lam,kw", [
    ("pendulum_N200_explore", "pendulum", 15, 200, 20.0, dict(exploration=0.3)),  # row 15: last float4 group partly used; padding lanes
    ("pendulum_N1000", "pendulum", 15, 1000, 20.0, {}),
    ("nav2d_N4288", "nav2d", 30, 4096 + 192, "ESSPS", _ESS(400.0)),              # several blocks, a partial last tile; device-resident temperature
    ("racing_N512", "racing", 25, 512, 50.0, {}),                                 # row 50
    ("cartpole_T200", "cartpole", 200, 512, "ESSPS", _ESS(150.0)),                # R = 50: two column chunks
    ("pendulum_saturated", "pendulum", 15, 1000, 20.0, dict(sigmas=[12.0])),       # sigma = 3 x (u_max - u_min): most U on a bound
])
def test_table_after_one_solve(name, model, T, N, lam, kw):
    solver, x0 = make(model, T, N, lam, adapt_covariance=True, **kw)
    assert np.array_equal(solver.sigma_seq.cpu().numpy(), np.tile(solver._sigmas.cpu().numpy(), (T, 1)))
    # a warm start off zero, so that the mean the solve sampled around is not the mean it stores
    mean = (np.random.default_rng(N).standard_normal((T, solver._dim_control)) * 0.2).astype(f32)
    solver.set_warm_start(mean)
    s = solve_and_check(name, solver, x0, None if lam == "ESSPS" else lam)
    if name == "pendulum_saturated":
        U = solver._perturbed_action_seqs.cpu().numpy()
        assert np.mean(np.abs(U) == 2.0) > 0.5
    assert s.shape == (T, solver._dim_control)


def test_generic_path_three_controls():
    """Opaque callables at dim_control = 3: the control index of a column depends on its float4 group (per-column tables);
    T * dc = 135 floats is two column chunks."""
    _need_gpu()
    from pi_mpc.mppi import MPPI

    T, N, dc = 45, 384, 3
    B = torch.tensor([[0.1, 0.0, 0.05], [0.0, 0.1, -0.05]], device="cuda")

    def dynamics(state, action):
        return state + action @ B.T

    def cost(state, action, info):
        return (state ** 2).sum(dim=1) + 0.05 * (action ** 2).sum(dim=1)

    solver = MPPI(horizon=T, num_samples=N, dim_state=2, dim_control=dc, dynamics=dynamics, cost_func=cost,
                  u_min=torch.tensor([-1.0, -0.5, -2.0]), u_max=torch.tensor([0.5, 0.6, 1.0]), sigmas=torch.tensor([0.5, 1.0, 2.0]),
                  lambda_=2.0, adapt_covariance=True, exploration=0.1)
    assert solver._model is None
    x0 = torch.tensor([1.0, -0.5])
    solve_and_check("generic_dc3", solver, x0, 2.0)
    solve_and_check("generic_dc3_second", solver, x0, 2.0)  # drawn from the adapted per-column table


# ------------------------------------------------------------------------------ 2. sparse and degenerate weights
def test_sparse_weights_racing():
    """racing at lambda = 1: one or two live tiles, every other tile is skipped."""
    solver, x0 = make("racing", 25, 4096, 1.0, adapt_covariance=True)
    solve_and_check("racing_sparse", solver, x0, 1.0)
    a, s = solver.forward(x0)
    assert torch.isfinite(a).all() and torch.isfinite(s).all()


@pytest.mark.parametrize("smin", [None, 0.05])
def test_one_sample_carries_all_the_weight(smin):
    """Costs set by hand, one sample far below the rest: var = 0 exactly, so s = sqrt(cov_floor), or sigma_min where larger."""
    T, N = 15, 300
    kw = {} if smin is None else dict(sigma_min=torch.tensor([smin]))
    solver, x0 = make("pendulum", T, N, 1.0, adapt_covariance=True, **kw)
    solver.forward(x0)
    h, st = solver._h, solver._stream()
    costs = torch.full((N,), 5000.0, device="cuda")
    costs[137] = 3.0
    a = torch.empty(T, 1, device="cuda")
    h.call("mppi_sample", 40, st)
    h.call("mppi_set_costs", costs.data_ptr(), 1, st)
    h.call("mppi_weights_reduce", 1.0, None, st)
    h.call("mppi_update_covariance", 1.0, st)
    h.call("mppi_finalize", None, 1, 1.0, 1, a.data_ptr(), None, None, st)
    want = np.sqrt(f32(1e-6)) if smin is None else f32(smin)
    assert np.array_equal(solver.sigma_seq.cpu().numpy(), np.full((T, 1), want, f32))
    solver._solve_idx = 41
    a2, s2 = solver.forward(x0)
    assert torch.isfinite(a2).all() and torch.isfinite(s2).all() and torch.isfinite(solver.sigma_seq).all()


# ------------------------------------------------------------------------------ 3. the next solve's noise
def test_next_solve_draws_z_times_table():
    """A twin with the same seed and sigmas = 1 exports z itself: the adaptive solver's noise of solve 2, and its posterior
    draw, are fl32(z * s[t,k]) bit for bit."""
    T, N = 30, 1000
    adaptive, x0 = make("nav2d", T, N, 100.0, adapt_covariance=True, sigma_min=torch.tensor([0.05, 0.05]))
    twin, _ = make("nav2d", T, N, 100.0, sigmas=[1.0, 1.0])
    for s in (adaptive, twin):
        s.forward(x0)
    table = adaptive.sigma_seq.cpu().numpy()
    assert not np.array_equal(table, np.tile(f32([0.5, 0.5]), (T, 1)))
    for s in (adaptive, twin):
        s.forward(x0)
    z = twin._action_noises.cpu().numpy()
    assert np.array_equal(adaptive._action_noises.cpu().numpy(), (z * table[None]).astype(f32))
    table = adaptive.sigma_seq.cpu().numpy()  # (solve 2 moved it again)
    loc = torch.zeros(T, 2)
    zq, _ = twin.get_samples_from_posterior(loc, x0, 64)
    got, _ = adaptive.get_samples_from_posterior(loc, x0, 64)
    assert np.array_equal(got.cpu().numpy(), (zq.cpu().numpy() * table[None]).astype(f32))


# ------------------------------------------------------------------------------ 4. cov_rate = 0 changes nothing
@pytest.mark.parametrize("model,T,N,lam", [("pendulum", 15, 1000, 20.0), ("racing", 50, 5000, 50.0)])
def test_rate_zero_is_the_default_solver(model, T, N, lam):
    """Three closed-loop solves: bit-identical action_seq, state_seq and costs, i.e. tiles drawn through the table are today's
    noise and the step with rate 0 never moves the table.  (The default solver is held to the multi-kernel sequence: the
    single launch of small problems sums the weighted rows in another order.)"""
    outs = []
    for adapt in (False, True):
        solver, x0 = make(model, T, N, lam, **(dict(adapt_covariance=True, cov_rate=0.0) if adapt else {}))
        solver.set_option("fused_solve", 0)
        x, rec = x0.cuda(), []
        for _ in range(3):
            a, s = solver.forward(x)
            rec += [a.clone(), s.clone(), solver._costs.clone()]
            x = s[0, 1].clone()
        rec.append(solver.sigma_seq.clone())
        outs.append(rec)
    for p, q in zip(*outs):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------ 5. closed loop
@pytest.mark.parametrize("lambda_", [100.0, "ESSPS"])
def test_closed_loop_with_filter_and_clamp(lambda_):
    """Five ticks, cov_rate = 0.5, sigma_min / sigma_max, Savitzky-Golay filter on: the table after every tick is the
    restatement iterated here (ubar is the UNFILTERED mean; clamp and smoothing compose), with a fixed temperature and with
    one read from the device (ESSPS)."""
    T, N = 30, 1024
    rule = dict(rate=0.5, floor=1e-4, smin=f32([0.2, 0.1]), smax=f32([0.45, 0.6]))
    solver, x0 = make("nav2d", T, N, lambda_, adapt_covariance=True, cov_rate=0.5, cov_floor=1e-4, use_sg_filter=True,
                      sigma_min=torch.tensor([0.2, 0.1]), sigma_max=torch.tensor([0.45, 0.6]),
                      **({} if lambda_ != "ESSPS" else dict(essps_target_ess=200.0, lambda_min=0.1, lambda_max=1000.0)))
    s = np.tile(f32([0.5, 0.5]), (T, 1)).astype(np.float64)
    x = x0.cuda()
    for tick in range(5):
        a, st = solver.forward(x)
        U, costs = solver._perturbed_action_seqs.cpu().numpy(), solver._costs.cpu().numpy()
        lam = float(solver._last_lambda)
        s = check_table(f"closed_loop_{lambda_}_tick{tick}", solver.sigma_seq.cpu().numpy(), U, costs, lam, s, **rule)
        assert np.all(s >= rule["smin"] - 1e-12) and np.all(s <= rule["smax"] + 1e-12)
        x = st[0, 1].clone()


# ------------------------------------------------------------------------------ 6. protocol
def _loop(solver, x, n):
    out = []
    for _ in range(n):
        a, s = solver.forward(x)
        out += [a.clone(), s.clone(), solver.sigma_seq.clone()]
        x = s[0, 1].clone()
    return out, x


def test_reset_deepcopy_state_dict_and_determinism():
    T, N = 15, 512
    kw = dict(adapt_covariance=True, cov_rate=0.7, sigma_min=torch.tensor([0.05]))
    a, x0 = make("pendulum", T, N, 20.0, **kw)
    b, _ = make("pendulum", T, N, 20.0, **kw)
    ra, xa = _loop(a, x0.cuda(), 2)
    rb, _ = _loop(b, x0.cuda(), 2)
    for p, q in zip(ra, rb):  # two identical solvers: bit-identical tables (the fold order is fixed)
        assert torch.equal(p, q)
    assert not torch.equal(a.sigma_seq, torch.ones(T, 1, device="cuda"))
    # deepcopy mid-loop and state_dict -> fresh solver -> load_state_dict continue bit-identically
    c = copy.deepcopy(a)
    d, _ = make("pendulum", T, N, 20.0, **kw)
    d.load_state_dict(a.state_dict())
    assert torch.equal(c.sigma_seq, a.sigma_seq) and torch.equal(d.sigma_seq, a.sigma_seq)
    ra2, _ = _loop(a, xa, 2)
    for other in (c, d):
        ro, _ = _loop(other, xa, 2)
        for p, q in zip(ra2, ro):
            assert torch.equal(p, q)
    # reset() puts the table back to the constructor's sigmas
    a.reset()
    assert torch.equal(a.sigma_seq, torch.ones(T, 1, device="cuda"))


def test_default_solver_has_no_drift_and_bad_arguments_raise():
    solver, x0 = make("nav2d", 30, 256, 100.0)
    for _ in range(2):
        solver.forward(x0)
    assert np.array_equal(solver.sigma_seq.cpu().numpy(), np.tile(f32([0.5, 0.5]), (30, 1)))
    with pytest.raises(ValueError):
        make("pendulum", 15, 100, 1.0, adapt_covariance=True, cov_rate=1.5)
    with pytest.raises(ValueError):
        make("nav2d", 30, 100, 1.0, adapt_covariance=True, sigma_min=torch.tensor([0.3, 0.1]), sigma_max=torch.tensor([0.2, 0.5]))
    with pytest.raises(ValueError, match="shard_samples"):
        make("pendulum", 15, 100, 1.0, adapt_covariance=True, shard_samples=True)
    with pytest.raises(ValueError, match="torch_cpu"):
        make("pendulum", 15, 100, 1.0, adapt_covariance=True, noise_source="torch_cpu")
