"""Temporally correlated sampling noise (noise_beta, mppi_set_noise_correlation) on a real MI355X.

The yardstick is the numpy restatement of tests/test_colored_noise_host.py: a twin solver with the same seed and sigmas = 1
exports the standard normals xi themselves, and the colored solver's noise must be fl32(z * s) bit for bit, with
z[0] = xi[0], z[t] = fl32(fl32(beta z[t-1]) + fl32(alpha xi[t])).
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import MODEL_CFG, orc
from test_colored_noise_host import restate

pytestmark = pytest.mark.gpu

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


def make_generic(dc, T, N, sigmas, lambda_=2.0, **kw):
    """(solver, start state) for a pair of opaque callables with dim_control = dc (the generic path)."""
    _need_gpu()
    from pi_mpc.mppi import MPPI

    B = (torch.arange(2 * dc, dtype=torch.float32).reshape(2, dc) % 3 - 1.0).cuda() * 0.05

    def dynamics(state, action):
        return state + action @ B.T

    def cost(state, action, info):
        return (state ** 2).sum(dim=1) + 0.05 * (action ** 2).sum(dim=1)

    solver = MPPI(horizon=T, num_samples=N, dim_state=2, dim_control=dc, dynamics=dynamics, cost_func=cost,
                  u_min=torch.full((dc,), -1.0), u_max=torch.full((dc,), 1.5), sigmas=torch.tensor(sigmas), lambda_=lambda_, **kw)
    assert solver._model is None
    return solver, torch.tensor([1.0, -0.5])


def colored(xi, beta, s):
    """eps[N,T,dc] of the rule from standard normals xi[N,T,dc], beta[dc] and s (sigmas[dc] or a table [T,dc])."""
    xi = np.asarray(xi, f32)
    N, T, dc = xi.shape
    beta = np.broadcast_to(np.asarray(beta, f32), (dc,))
    z = np.empty_like(xi)
    for k in range(dc):
        z[:, :, k] = restate(xi[:, :, k], beta[k])
    return (z * np.broadcast_to(np.asarray(s, f32), (T, dc))[None]).astype(f32)


# ------------------------------------------------------------------------------ 1. the tiles equal the rule
def _pair(case, T, N):
    """(colored solver, twin with sigmas = 1 and no filter, start state, beta[dc], sigmas[dc])."""
    if case == "pendulum":      # dc = 1: the recurrence runs inside a float4 group and across groups
        beta, sig = [0.9], [0.7]
        a, x0 = make("pendulum", T, N, 20.0, sigmas=sig, noise_beta=0.9)
        b, _ = make("pendulum", T, N, 20.0, sigmas=[1.0])
    elif case == "nav2d":       # dc = 2: two interleaved chains
        beta, sig = [0.9, 0.3], [0.5, 0.25]
        a, x0 = make("nav2d", T, N, 100.0, sigmas=sig, noise_beta=beta)
        b, _ = make("nav2d", T, N, 100.0, sigmas=[1.0, 1.0])
    elif case == "generic3":    # a wide handle (per-column tables), a zero entry among non-zero ones
        beta, sig = [0.5, 0.9, 0.0], [0.5, 1.0, 2.0]
        a, x0 = make_generic(3, T, N, sig, noise_beta=torch.tensor(beta))
        b, _ = make_generic(3, T, N, [1.0] * 3)
    elif case == "generic4":    # one step per group
        beta, sig = [0.9] * 4, [0.5, 1.0, 2.0, 0.25]
        a, x0 = make_generic(4, T, N, sig, noise_beta=0.9)
        b, _ = make_generic(4, T, N, [1.0] * 4)
    else:                       # dim_control = 6: rows wider than a group, the lane reads its earlier columns back
        beta, sig = [0.9, 0.5, 0.0, 0.99, 0.3, 0.7], [0.5, 1.0, 2.0, 0.25, 0.1, 1.5]
        a, x0 = make_generic(6, T, N, sig, noise_beta=beta)
        b, _ = make_generic(6, T, N, [1.0] * 6)
    return a, b, x0, f32(beta), f32(sig)


@pytest.mark.parametrize("case,T,N", [
    ("pendulum", 1, 100), ("pendulum", 5, 321), ("pendulum", 8, 100), ("pendulum", 8, 321), ("pendulum", 5, 100), ("pendulum", 1, 321),
    ("nav2d", 3, 100), ("nav2d", 16, 321), ("nav2d", 3, 321), ("nav2d", 16, 100),
    ("generic3", 5, 130),
    ("generic4", 3, 64),
    ("generic6", 5, 130),
])
def test_tiles_equal_the_rule(case, T, N):
    """No recurrence (T = 1), a ragged last group, a partial tile, a partial last block, every carry width — two consecutive
    solves (the filter restarts every solve, the stream advances) and a posterior draw."""
    a, b, x0, beta, sig = _pair(case, T, N)
    assert np.array_equal(a.noise_beta.numpy(), beta)
    seen = []
    for _ in range(2):
        a.forward(x0)
        b.forward(x0)
        xi = b._action_noises.cpu().numpy()
        got = a._action_noises.cpu().numpy()
        assert np.all(np.isfinite(got))
        assert np.array_equal(got, colored(xi, beta, sig))
        seen.append(xi)
    assert not np.array_equal(seen[0], seen[1])
    if T > 1:  # the filter did something: not the unfiltered noise
        assert not np.array_equal(got, (xi * sig[None, None]).astype(f32))
    loc = torch.zeros(T, len(sig))
    xq, _ = b.get_samples_from_posterior(loc, x0, 64)
    gq, _ = a.get_samples_from_posterior(loc, x0, 64)
    assert np.array_equal(gq.cpu().numpy(), colored(xq.cpu().numpy(), beta, sig))
    assert a._solve_idx == b._solve_idx  # the filtered and the unfiltered stream consume the same normals


# ------------------------------------------------------------------------------ 2. statistics of the device stream
def test_device_stream_is_stationary():
    """eps / sigma per (t, k): variance 1 and lag-1 correlation beta, to six standard deviations of the two estimators."""
    N, T, beta = 65536, 8, 0.9
    solver, x0 = make("nav2d", T, N, 100.0, noise_beta=beta)
    solver.forward(x0)
    z = solver._action_noises.cpu().numpy().astype(np.float64) / 0.5
    var_lim, cor_lim = 6.0 * np.sqrt(2.0 / N), 6.0 * np.sqrt((1.0 + beta * beta) / N)
    for k in range(2):
        for t in range(T):
            dv = abs(np.mean(z[:, t, k] ** 2) - 1.0)
            dc = abs(np.mean(z[:, t, k] * z[:, t - 1, k]) - beta) if t else 0.0
            print(f"[colored] k {k} t {t}: |var - 1| {dv:.4f} (limit {var_lim:.4f}), |corr - beta| {dc:.4f} (limit {cor_lim:.4f})")
            assert dv <= var_lim
            assert dc <= cor_lim


# ------------------------------------------------------------------------------ 3. every consumer reads the colored tiles
def _consumer_pair(model):
    if model == "racing":
        return [make("racing", 12, 1000, 50.0, **kw) for kw in (dict(noise_beta=0.9), {})]
    if model == "pendulum":
        rule = dict(essps_target_ess=100.0, lambda_min=1e-3, lambda_max=1e5)
        return [make("pendulum", 15, 1000, "ESSPS", **rule, **kw) for kw in (dict(noise_beta=0.9), {})]
    return [make_generic(3, 5, 130, [0.5, 1.0, 2.0], **kw) for kw in (dict(noise_beta=[0.5, 0.9, 0.0]), {})]


@pytest.mark.parametrize("model", ["racing", "pendulum", "generic3"])
def test_every_consumer_reads_the_colored_tiles(model):
    """Three closed-loop solves; in lockstep a default solver into which each solve's exported colored noise is injected.  Both
    take the tile path through the same kernels: identical plans, states, costs, temperatures and top samples."""
    (a, x0), (b, _) = _consumer_pair(model)
    x = x0.cuda()
    for tick in range(3):
        act, seq = a.forward(x)
        eps = a._action_noises
        b.inject_noise(eps)
        act_b, seq_b = b.forward(x)
        assert torch.equal(act, act_b), tick
        assert torch.equal(seq, seq_b), tick
        assert torch.equal(a._costs, b._costs), tick
        assert float(a._lambda) == float(b._lambda) and float(a._last_lambda) == float(b._last_lambda)
        (sa, wa), (sb, wb) = a.get_top_samples(8), b.get_top_samples(8)
        assert torch.equal(sa, sb) and torch.equal(wa, wb), tick
        assert torch.isfinite(act).all() and torch.isfinite(seq).all()
        x = seq[0, 1].clone()


# ------------------------------------------------------------------------------ 4. with the covariance adaptation
def test_with_covariance_adaptation():
    """The filter runs on the standard normals and the adapted table scales after it: the noise of solve 2 is fl32(z * table)."""
    T, N, beta = 30, 1000, 0.8
    a, x0 = make("nav2d", T, N, 100.0, adapt_covariance=True, sigma_min=torch.tensor([0.05, 0.05]), noise_beta=beta)
    twin, _ = make("nav2d", T, N, 100.0, sigmas=[1.0, 1.0])
    for s in (a, twin):
        s.forward(x0)
    table = a.sigma_seq.cpu().numpy()
    assert not np.array_equal(table, np.tile(f32([0.5, 0.5]), (T, 1)))
    for s in (a, twin):
        s.forward(x0)
    xi = twin._action_noises.cpu().numpy()
    assert np.array_equal(a._action_noises.cpu().numpy(), colored(xi, [beta, beta], table))


# ------------------------------------------------------------------------------ 5. shard invariance at the C ABI
def _generic_handle(N, offset, inherit, T=5, dc=2, seed=42):
    from mppi_playground_amd import _capi

    f4 = lambda *v: (C.c_float * 4)(*v)  # noqa: E731
    cfg = _capi.MppiConfig(model=_capi.MODEL_GENERIC, horizon=T, dim_state=2, dim_control=dc, num_samples=N, sample_offset=offset,
                           inherit_count=inherit, u_min=f4(-1, -1, -1, -1), u_max=f4(1, 1, 1, 1), sigmas=f4(0.5, 0.25, 1.0, 2.0),
                           seed=seed, device=0)
    return _capi.Handle(cfg)


def _export(h, N, T, dc, solve_idx):
    e = torch.empty(N, T, dc, device="cuda")
    h.call("mppi_sample", solve_idx, None)
    h.call("mppi_export_noise", e.data_ptr(), None, None)
    torch.cuda.synchronize()
    return e.cpu().numpy()


def test_shard_invariance_at_the_c_abi():
    """The filter never crosses samples and the counter is the global sample index: a shard's rows are the unsharded rows."""
    _need_gpu()
    T, dc = 5, 2
    beta = (C.c_float * dc)(0.9, 0.3)
    full, part = _generic_handle(192, 0, 150), _generic_handle(64, 128, 150)
    for h in (full, part):
        h.call("mppi_set_noise_correlation", beta)
    e_full, e_part = _export(full, 192, T, dc, 3), _export(part, 64, T, dc, 3)
    assert np.array_equal(e_part, e_full[128:192])
    plain = _generic_handle(192, 0, 150)
    assert not np.array_equal(_export(plain, 192, T, dc, 3), e_full)


# ------------------------------------------------------------------------------ 6. protocol
def _loop(solver, x, n):
    out = []
    for _ in range(n):
        a, s = solver.forward(x)
        out += [a.clone(), s.clone(), solver._action_noises.clone()]
        x = s[0, 1].clone()
    return out, x


def test_deepcopy_and_state_dict_continue_bit_equal():
    T, N = 15, 512
    kw = dict(noise_beta=0.85)
    a, x0 = make("pendulum", T, N, 20.0, **kw)
    _, xa = _loop(a, x0.cuda(), 2)
    c = copy.deepcopy(a)
    d, _ = make("pendulum", T, N, 20.0)  # a default solver: the state dict carries the setting
    d.load_state_dict(a.state_dict())
    for other in (c, d):
        assert np.array_equal(other.noise_beta.numpy(), f32([0.85]))
    ra, _ = _loop(a, xa, 2)
    for other in (c, d):
        ro, _ = _loop(other, xa, 2)
        for p, q in zip(ra, ro):
            assert torch.equal(p, q)
    a.reset()  # leaves the setting alone
    assert np.array_equal(a.noise_beta.numpy(), f32([0.85]))
    e = copy.deepcopy(d)  # a copy of a solver whose setting was changed after construction
    assert np.array_equal(e.noise_beta.numpy(), f32([0.85]))


def test_clone_state_carries_the_setting():
    _need_gpu()
    src, dst = _generic_handle(64, 0, 64), _generic_handle(64, 0, 64)
    src.call("mppi_set_noise_correlation", (C.c_float * 2)(0.9, 0.3))
    assert src.lib.mppi_clone_state(dst.h, src.h) == 0
    got = (C.c_float * 2)()
    dst.call("mppi_get_noise_correlation", got)
    assert list(got) == [f32(0.9), f32(0.3)]
    assert np.array_equal(_export(dst, 64, 5, 2, 7), _export(src, 64, 5, 2, 7))
    src.call("mppi_set_noise_correlation", None)  # ... and its absence
    assert src.lib.mppi_clone_state(dst.h, src.h) == 0
    dst.call("mppi_get_noise_correlation", got)
    assert list(got) == [0.0, 0.0]
    assert np.array_equal(_export(dst, 64, 5, 2, 8), _export(_generic_handle(64, 0, 64), 64, 5, 2, 8))


def _geometry(solver):
    blocks, spb = C.c_int(-1), C.c_int(-1)
    solver._h.call("mppi_fused_geometry", C.byref(blocks), C.byref(spb))
    return blocks.value, spb.value


def test_set_noise_beta_zero_returns_to_the_default_noise_and_the_single_launch():
    T, N = 15, 1000
    a, x0 = make("pendulum", T, N, 20.0, noise_beta=0.9)
    twin, _ = make("pendulum", T, N, 20.0)
    for s in (a, twin):
        s.forward(x0)
    assert _geometry(a) == (0, 0)      # the single launch regenerates its noise: a colored solve takes the multi-kernel sequence
    assert _geometry(twin)[0] > 0
    assert not torch.equal(a._action_noises, twin._action_noises)
    a.set_noise_beta(0)
    assert not a.noise_beta.any()
    for s in (a, twin):
        s.forward(x0)
    assert torch.equal(a._action_noises, twin._action_noises)
    assert _geometry(a) == _geometry(twin) and _geometry(a)[0] > 0
    a.set_noise_beta([0.5])
    a.forward(x0)
    assert _geometry(a) == (0, 0)


# ------------------------------------------------------------------------------ 7. errors
def test_bad_arguments_raise():
    _need_gpu()
    with pytest.raises(ValueError):
        make("pendulum", 15, 100, 1.0, noise_beta=1.0)
    with pytest.raises(ValueError):
        make("pendulum", 15, 100, 1.0, noise_beta=-0.1)
    with pytest.raises(ValueError):
        make("nav2d", 30, 100, 1.0, noise_beta=[0.5])
    with pytest.raises(ValueError, match="torch_cpu"):
        make("pendulum", 15, 100, 1.0, noise_beta=0.5, noise_source="torch_cpu")
    with pytest.raises(ValueError, match="action_cost"):
        make("pendulum", 15, 100, 1.0, noise_beta=0.5, action_cost=True)
    solver, _ = make("pendulum", 15, 100, 1.0)
    with pytest.raises(ValueError):
        solver.set_noise_beta(1.0)
    h = _generic_handle(64, 0, 64)
    for bad in ((1.0, 0.5), (0.5, -0.1), (float("nan"), 0.0)):
        rc = h.lib.mppi_set_noise_correlation(h.h, (C.c_float * 2)(*bad))
        assert rc == -1  # MPPI_E_INVALID
        assert b"beta" in h.lib.mppi_last_error(h.h)
    got = (C.c_float * 2)(7.0, 7.0)
    h.call("mppi_get_noise_correlation", got)
    assert list(got) == [0.0, 0.0]  # a refused call leaves the setting alone
