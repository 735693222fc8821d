"""The two soft disc models (MPPI_MODEL_NAV2D_DISCS_SOFT / MPPI_MODEL_RACING_DISCS_SOFT: mppi_set_disc_softness,
envs.SoftMovingObstacleNav2DEnv, envs.racing_opponents' Soft classes) on a real MI355X.

The rigs are those of test_gpu_moving_discs.py / test_gpu_racing_discs.py around the soft classes; the reference is
tests/soft_discs_ref.py on the EXPORTED actions and the DEVICE'S OWN state sequences (mppi_rollout_samples), with the case
tables the CPU suite has held to their claims under the soft rule (test_soft_discs_host.py).

  math 0    every sample's cost equals, BIT FOR BIT, the fp32 restatement on the device's states (every operation of the rule
            — subtract, multiply, add, the IEEE quotient, max, compare — is exactly rounded everywhere).
  math 1, 2 the parity rule — 2e-6 of the cost scale — against the float64 restatement on the same states (soft_discs_ref says
            why the same states: a ramp's slope multiplies the fp32 rounding of a position, a flat indicator does not), for every
            sample the boundary rule keeps; with skirt = 1 the penalty is continuous at the rim and only `edge` samples are left
            out.  The device's reciprocal is 1 ulp: the CPU suite keeps the fp32 restatement within a quarter of the rule.
  skirt = 0 a soft handle equals a hard-model handle on the same seed and table bit for bit, at every math level.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import action_cost_ref as acref
import discs_ref as D
import racing_discs_ref as RD
import soft_discs_ref as R
import test_gpu_moving_discs as NAV
import test_gpu_racing_discs as RAC
from test_gpu_action_cost import LAM, Rig, measure, term
from test_gpu_covariance import _need_gpu, weights64
from test_gpu_fused_geometry import ALL_INHERIT, took

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
MODELS = ("nav2d", "racing")
NAMES = {"nav2d": "nav2d_discs_soft", "racing": "racing_discs_soft"}
E_INVALID = -1
_envs = {}
same_bits, bits = NAV.same_bits, NAV.bits


def env_for(model, T):
    _need_gpu()
    from envs import SoftMovingObstacleNav2DEnv
    from envs.racing_opponents import SoftOpponentRacingEnv

    if (model, T) not in _envs:
        _envs[model, T] = SoftMovingObstacleNav2DEnv(horizon=T) if model == "nav2d" else SoftOpponentRacingEnv(horizon=T)
    return _envs[model, T]


def case(model, name, T):
    """-> (table, x0, ref or None)"""
    if model == "nav2d":
        table, x0 = D.case(name, T)
        return table, x0, None
    return RAC.case(name, T)


def nav_solver(env, T, N, lam=1.0, tag=True, **kw):
    from pi_mpc.mppi import MPPI

    dyn, cost = (env.dynamics, env.cost_function) if tag else ((lambda s, a: env.dynamics(s, a)), (lambda s, a, i: env.cost_function(s, a, i)))
    solver = MPPI(horizon=T, num_samples=N, dim_state=3, dim_control=2, dynamics=dyn, cost_func=cost, u_min=torch.tensor(D.U_MIN),
                  u_max=torch.tensor(D.U_MAX), sigmas=torch.tensor(D.SIGMAS), lambda_=lam, **kw)
    assert (solver._model == "nav2d_discs_soft") if tag else (solver._model is None)
    return solver


def racing_ctrl(env, T, N, ref, lam=1.0, **kw):
    from envs.racing_opponents import soft_opponent_racing_controller

    ctrl = soft_opponent_racing_controller(env, horizon=T, num_samples=N, lambda_=lam, **kw)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    ctrl.set_reference(ref)
    ctrl.solver._test_keep = ctrl
    assert ctrl.solver._model == "racing_discs_soft"
    return ctrl


def racing_untagged(env, T, N, ref, lam=1.0, **kw):
    from pi_mpc.mppi import MPPI

    ctrl = racing_ctrl(env, T, 64, ref)
    solver = MPPI(horizon=T, num_samples=N, dim_state=4, dim_control=2, dynamics=lambda s, a: env.dynamics(s, a),
                  cost_func=lambda s, a, i: ctrl.cost_function(s, a, i), u_min=env.u_min, u_max=env.u_max,
                  sigmas=torch.tensor(RD.SIGMAS), lambda_=lam, **kw)
    assert solver._model is None
    solver._test_keep = ctrl
    return solver


def solver_for(model, env, T, N, ref, tag=True, **kw):
    if model == "nav2d":
        return nav_solver(env, T, N, tag=tag, **kw)
    return racing_ctrl(env, T, N, ref, **kw).solver if tag else racing_untagged(env, T, N, ref, **kw)


def put_table(model, env, table):
    (NAV if model == "nav2d" else RAC).put_table(env, table)


class _Soft:
    """what the two soft rigs share: the pair on the env and on the handle, the soft restatement, a handle of the soft id"""

    def _finish(self, x0, T, setting, math, mode):
        self.x0_host = f32(x0)
        self.h.call("mppi_set_option", b"math", math)
        if mode is not None:
            self.h.call("mppi_set_option", b"fused_solve", mode)
        ref = D if self.kind == "nav2d" else RD
        self.mean0 = np.broadcast_to(ref.MEAN, (T, 2)).copy()
        self.set_mean(self.mean0)
        self.ab = R.coefficients(*setting)

    def set_softness(self, reach, skirt):
        """through the C ABI, between launches; the env is told too, so that a later forward() does not put its own pair back"""
        self.env.set_softness(reach, skirt)
        self.h.call("mppi_set_disc_softness", float(reach), float(skirt))
        self.h.soft_key = (float(reach), float(skirt))
        self.ab = R.coefficients(reach, skirt)

    def soft_cfg(self, n, offset, inherit):
        from mppi_playground_amd import _capi

        ref = D if self.kind == "nav2d" else RD
        cfg = _capi.MppiConfig()
        cfg.model = _capi.MODEL_IDS[NAMES[self.kind]]
        cfg.horizon, cfg.dim_state, cfg.dim_control = self.T, self.ds, 2
        cfg.num_samples, cfg.sample_offset = n, int(offset)
        cfg.inherit_count = ALL_INHERIT if inherit is None else int(inherit)
        for k in range(2):
            cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = float(ref.U_MIN[k]), float(ref.U_MAX[k]), float(ref.SIGMAS[k])
        cfg.seed, cfg.device = self.solver._seed, 0
        sol = self.solver
        sol._h.close()
        sol._h = _capi.Handle(cfg)
        sol._uploaded, sol._params_set, sol._ref_uploaded = {}, None, None


class SoftNavRig(_Soft, NAV.DiscRig):
    kind = "nav2d"

    def __init__(self, table, x0, ref, T, N, setting=(2.0, 1.0), math=0, mode=None, **kw):
        self.env = env_for("nav2d", T)
        self.env.set_softness(*setting)
        self.table = np.ascontiguousarray(table, f32)
        NAV.put_table(self.env, self.table)
        self.P, self.grid = NAV.world(self.env)
        Rig.__init__(self, "nav2d_discs_soft", T, N, solver=(nav_solver(self.env, T, N, **kw), torch.from_numpy(f32(x0).copy())))
        self._finish(x0, T, setting, math, mode)

    def window(self, offset, inherit=None):
        self.soft_cfg(self.N, offset, inherit)
        self._prepare()

    def ref(self, U, dtype=f32, **kw):
        return R.rollout_nav2d(self.P, self.grid, self.table, self.x0_host, U, self.ab[0], self.ab[1], dtype, **kw)


class SoftRacingRig(_Soft, RAC.DiscRig):
    kind = "racing"

    def __init__(self, table, x0, ref, T, N, setting=(2.0, 1.0), math=0, mode=None, **kw):
        self.env = env_for("racing", T)
        self.env.set_softness(*setting)
        self.table = np.ascontiguousarray(table, f32)
        self.ref_path = np.ascontiguousarray(ref, f32)
        RAC.put_table(self.env, self.table)
        self.ctrl = racing_ctrl(self.env, T, N, self.ref_path, **kw)
        self.P, self.grids = RAC.world(self.ctrl)
        Rig.__init__(self, "racing_discs_soft", T, N, solver=(self.ctrl.solver, torch.from_numpy(f32(x0).copy())))
        self._finish(x0, T, setting, math, mode)

    def new_handle(self, offset=0, inherit=None, n=None):
        self.soft_cfg(self.N if n is None else n, offset, inherit)

    def ref(self, U, dtype=f32, **kw):
        return R.rollout_racing(self.P, self.grids, self.ref_path, self.table, self.x0_host, U, self.ab[0], self.ab[1], dtype, **kw)


def soft_rig(model, name, T, N, **kw):
    return (SoftNavRig if model == "nav2d" else SoftRacingRig)(*case(model, name, T), T, N, **kw)


def hard_rig(model, name, T, N, **kw):
    table, x0, ref = case(model, name, T)
    return NAV.DiscRig(table, x0, T, N, **kw) if model == "nav2d" else RAC.DiscRig(table, x0, ref, T, N, **kw)


def plain_rig(model, name, T, N, mean, **kw):
    table, x0, ref = case(model, name, T)
    return NAV.plain_rig(T, N, x0, mean, **kw) if model == "nav2d" else RAC.plain_rig(T, N, x0, ref, mean, **kw)


def level0(name, rig, c, U, S):
    own = rig.ref(U, states=S)
    same_bits(f"{name}: costs against the fp32 restatement on the device's states", c, own["costs"])
    return own


def in_parity(name, rig, c, U, S):
    """the parity rule against float64 on the device's own states; skirt = 1: only `edge` samples are left out"""
    r64 = rig.ref(U, f64, states=S)
    left = int(r64["near"].sum())
    keep = ~r64["edge"] if rig.env.soft_skirt == 1.0 else ~(r64["near"] | r64["edge"])
    err = np.abs(c.astype(f64) - r64["costs"])
    worst = float(err[keep].max() / r64["scale"]) if keep.any() else 0.0
    print(f"[soft discs] {name}: left out {int((~keep).sum())} ({left} at a rim, cap {R.cap(len(c))}); max err {worst:.3g} of the scale; "
          f"skirt share {float(r64['skirted'].any(axis=(1, 2)).mean()) if r64['skirted'].size else 0.0:.3f}")
    assert np.all(np.isfinite(c)), name
    assert left <= R.cap(len(c)), f"{name}: the boundary rule leaves out {left} samples"
    assert worst <= R.PARITY, f"{name}: {worst:.3g} of the scale against {R.PARITY}"
    return r64


def case_names(model):
    return list((D if model == "nav2d" else RD).CASES)


ALL_CASES = [(m, n) for m in MODELS for n in case_names(m)]


# ------------------------------------------------------------------------------ 1. math 0: bit for bit
@pytest.mark.parametrize("model,name", ALL_CASES)
def test_math0_costs_bit_for_bit(model, name):
    skirted = 0.0
    for T in R.HORIZONS:
        for N in (100, 4160):
            rig = soft_rig(model, name, T, N)
            S = U = None
            for setting in ((2.0, 0.25), (2.0, 1.0)):
                rig.set_softness(*setting)
                c = rig.rollout(3)
                if S is None:  # (the re-roll is dynamics only and the noise is the solve index's: once per rig)
                    U, S = rig.actions_around(rig.mean0), rig.states()
                own = level0(f"{model} {name} T{T} N{N} {setting}", rig, c, U, S)
                skirted = max(skirted, float(own["skirted"].any(axis=(1, 2)).mean()) if own["skirted"].size else 0.0)
            rig.close()
    if name in (D.MIXED if model == "nav2d" else RD.MIXED):
        assert skirted >= 0.05  # the ramp was exercised


# ------------------------------------------------------------------------------ 2. the fast levels: the parity rule
@pytest.mark.parametrize("math", [1, 2])
@pytest.mark.parametrize("model,name", ALL_CASES)
def test_fast_levels_within_the_parity_rule(model, name, math):
    for T in R.HORIZONS + ((R.T_LONG,) if name in ("n8", "terminal") else ()):
        for N in (100, 4160):
            if T == R.T_LONG and N != 100:
                continue
            rig = soft_rig(model, name, T, N, math=math)
            S = U = None
            for setting in ((2.0, 1.0), (2.0, 0.25)):
                rig.set_softness(*setting)
                c = rig.rollout(5)
                if S is None:
                    U, S = rig.actions_around(rig.mean0), rig.states()
                in_parity(f"{model} {name} math {math} T{T} N{N} {setting}", rig, c, U, S)
            rig.close()


# ------------------------------------------------------------------------------ 3. skirt = 0 against the hard model
@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("model", MODELS)
def test_skirt_zero_equals_the_hard_model(model, math):
    for T in (7, 8, 25):
        for N in (100, 4160):
            a = soft_rig(model, "n3", T, N, setting=R.HARD, math=math)
            b = hard_rig(model, "n3", T, N, math=math)
            (aa, sa, _, ca), (ab, sb, _, cb) = a.solve(2, 5.0), b.solve(2, 5.0)
            tagname = f"{model} math {math} T{T} N{N}"
            same_bits(f"{tagname} costs", ca, cb)
            same_bits(f"{tagname} action_seq", aa, ab)
            same_bits(f"{tagname} state_seq", sa, sb)
            if T == 8 and N == 100:  # (the discs are charged: a soft setting moves the costs)
                a.set_softness(2.0, 1.0)
                a.set_mean(a.mean0)
                assert not np.array_equal(a.solve(2, 5.0)[3], cb)
            a.close()
            b.close()


# ------------------------------------------------------------------------------ 4. n = 0 against the plain model
@pytest.mark.parametrize("model", MODELS)
def test_no_discs_equals_the_plain_model(model):
    for T in (7, 8):
        N = 1000
        a = soft_rig(model, "n0", T, N, setting=(3.0, 0.5), math=2)
        b = plain_rig(model, "n0", T, N, a.mean0, math=2)
        (aa, sa, _, ca), (ab, sb, _, cb) = a.solve(1, 5.0), b.solve(1, 5.0)
        same_bits(f"{model} T{T} costs", ca, cb)
        same_bits(f"{model} T{T} action_seq", aa, ab)
        same_bits(f"{model} T{T} state_seq", sa, sb)
        a.close()
        b.close()


# ------------------------------------------------------------------------------ 5. every launch path on one mixed case
@pytest.mark.parametrize("model", MODELS)
def test_every_launch_path_agrees(model):
    T, N, setting = 8, 1000, (2.0, 0.25)
    mk = soft_rig(model, "n3", T, N, setting=setting, mode=0)
    a0, s0, _, c0 = mk.solve(4, 5.0)
    assert took(mk.h) == (0, 0)
    U, S = mk.actions_around(mk.mean0), mk.states()
    own = level0(f"{model} n3 multi-kernel", mk, c0, U, S)
    assert own["skirted"].any(axis=(1, 2)).mean() >= 0.05
    sl = soft_rig(model, "n3", T, N, setting=setting)
    a1, s1, _, c1 = sl.solve(4, 5.0)
    assert took(sl.h) != (0, 0)
    same_bits("single launch costs", c1, c0)
    assert np.max(np.abs(a1 - a0)) <= 1e-5 and np.max(np.abs(s1 - s0)) <= 1e-4  # (another order of the weighted sums)
    sl.set_mean(sl.mean0)                             # (the solve left its warm start there)
    sl.h.call("mppi_set_option", b"noise_regen", 0)   # materialised tiles against noise regenerated in registers
    same_bits("tiles", sl.rollout(4), c0)
    sl.h.call("mppi_set_option", b"noise_regen", 1)
    same_bits("regenerated", sl.rollout(4), c0)
    # the top-k re-roll: the winners' states are the re-rolled states of those samples, in the order of these costs
    k = 8
    st, w = torch.empty(k, T + 1, S.shape[2], device="cuda"), torch.empty(k, device="cuda")
    mk.h.call("mppi_top_samples", k, 5.0, st.data_ptr(), w.data_ptr(), mk.solver._stream())
    torch.cuda.synchronize()
    assert np.all(np.diff(w.cpu().numpy()) <= 0)
    order = np.argsort(c0, kind="stable")
    top = st.cpu().numpy()
    if len(np.unique(c0[order[:k + 1]])) == k + 1:  # no ties around the cut: the order is determined
        same_bits("top states", top, S[order[:k]])
    else:
        cand = S[c0 <= c0[order[k - 1]]]
        for row in top:
            assert any(np.array_equal(bits(row), bits(x)) for x in cand)
    mk.close()
    sl.close()


@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("model", MODELS)
def test_wavefront_per_trajectory_mapping(model, math):
    rig = soft_rig(model, "n3", 8, 100, setting=(2.0, 0.25), math=math)
    rig.h.call("mppi_set_option", b"mapping", 1)
    c = rig.rollout(6)
    in_parity(f"{model} n3 math {math} mapping 1", rig, c, rig.actions_around(rig.mean0), rig.states())
    rig.close()


@pytest.mark.parametrize("model", MODELS)
def test_lazy_state_seq_through_forward(model):
    T, N = 8, 1000
    table, x0, ref = case(model, "n3", T)
    env = env_for(model, T)
    env.set_softness(2.0, 0.25)
    put_table(model, env, table)
    outs = []
    for lazy in (False, True):
        solver = solver_for(model, env, T, N, ref, lam=5.0, lazy_state_seq=lazy)
        x = torch.from_numpy(f32(x0).copy()).cuda()
        seq = []
        for k in range(3):
            if k == 2:
                env.set_softness(3.0, 0.5)  # settles the pending state sequence of solve 1 with ITS constants first
            a, s = solver.forward(x)
            seq.append((a.cpu().numpy().copy(), s.cpu().numpy().copy(), solver._costs.cpu().numpy().copy()))
            x = s[0, 1].clone()
        env.set_softness(2.0, 0.25)
        outs.append(seq)
    for (a0, s0, c0), (a1, s1, c1) in zip(*outs):
        same_bits("lazy costs", c1, c0)
        same_bits("lazy action_seq", a1, a0)
        same_bits("lazy state_seq", s1, s0)


@pytest.mark.parametrize("model", MODELS)
def test_control_cost_instantiation_equals_the_separate_pass(model):
    T, N = 8, 200
    rig = soft_rig(model, "n3", T, N, setting=(2.0, 0.25), math=2)
    ref = D if model == "nav2d" else RD
    mean = np.random.default_rng(7).uniform(ref.U_MIN, ref.U_MAX, (T, 2)).astype(f32)
    c0, c1, U, g = measure(f"{NAMES[model]}_in_rollout", rig, idx=7, mean=mean, sig=ref.SIGMAS)
    term(rig, 0.0)
    assert np.array_equal(rig.rollout(7), c0)
    term(rig, 1.0)
    rig.h.call("mppi_add_action_cost", LAM, rig.solver._stream())
    added = rig.costs()
    acref.check(f"{NAMES[model]}_separate_pass", added, c0, acref.kappa32(1.0, LAM), g, U)
    same_bits("separate pass", added, c1)
    rig.close()


# ------------------------------------------------------------------------------ 6. the pair's hand-over
@pytest.mark.parametrize("model", MODELS)
def test_softness_handover_in_stream_order(model):
    T, N = 8, 1000
    rig = soft_rig(model, "n3", T, N, math=2)
    reach, skirt = C.c_float(-1.0), C.c_float(-1.0)
    rig.h.call("mppi_get_disc_softness", C.byref(reach), C.byref(skirt))
    assert (reach.value, skirt.value) == (2.0, 1.0)  # what a soft handle starts at
    _, _, _, first = rig.solve(1, 5.0)
    rig.set_mean(rig.mean0)
    rig.h.call("mppi_set_disc_softness", 3.0, 0.5)   # (no synchronisation in between: stream order)
    _, _, _, second = rig.solve(2, 5.0)
    rig.h.call("mppi_get_disc_softness", C.byref(reach), C.byref(skirt))
    assert (reach.value, skirt.value) == (3.0, 0.5)
    rig.h.call("mppi_get_disc_softness", None, C.byref(skirt))
    rig.close()
    a = soft_rig(model, "n3", T, N, math=2)
    same_bits("first solve: the starting pair", first, a.solve(1, 5.0)[3])
    a.set_mean(a.mean0)
    assert not np.array_equal(second, a.solve(2, 5.0)[3])  # the new pair moved the second solve
    a.close()
    b = soft_rig(model, "n3", T, N, setting=(3.0, 0.5), math=2)
    same_bits("second solve: the new pair", second, b.solve(2, 5.0)[3])
    twin = soft_rig(model, "n3", T, N, math=2)           # mppi_clone_state carries the pair
    assert twin.h.lib.mppi_clone_state(twin.h.h, b.h.h) == 0
    twin.h.call("mppi_get_disc_softness", C.byref(reach), C.byref(skirt))
    assert (reach.value, skirt.value) == (3.0, 0.5)
    twin.set_mean(twin.mean0)
    b.set_mean(b.mean0)
    same_bits("a clone's costs", twin.rollout(3), b.rollout(3))
    twin.close()
    b.close()


@pytest.mark.parametrize("rule", ["ESSPS", "LBPS"])
@pytest.mark.parametrize("model", MODELS)
def test_temperature_rules_run_on_a_soft_handle(model, rule):
    T, N = 8, 1000
    table, x0, ref = case(model, "n3", T)
    env = env_for(model, T)
    env.set_softness(2.0, 1.0)
    put_table(model, env, table)
    solver = solver_for(model, env, T, N, ref, lam=rule)
    assert solver._rule_on_device == rule
    x = torch.from_numpy(f32(x0).copy()).cuda()
    for _ in range(2):
        a, s = solver.forward(x)
        x = s[0, 1].clone()
    lam = float(solver._lambda)
    assert np.isfinite(lam) and solver._lambda_min <= lam <= solver._lambda_max
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(s).all()) and bool(torch.isfinite(solver._costs).all())


# ------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("model", MODELS)
def test_refusals(model):
    T, N = 8, 64
    table, x0, ref = case(model, "n3", T)
    rig = soft_rig(model, "n3", T, N)
    lib, h, st = rig.h.lib, rig.h.h, rig.solver._stream()
    want = rig.rollout(3)
    for reach in (1.0, 0.5, float("nan"), float("inf")):
        assert lib.mppi_set_disc_softness(h, C.c_float(reach), C.c_float(0.5)) == E_INVALID, reach
    for skirt in (-0.1, 1.1, float("nan")):
        assert lib.mppi_set_disc_softness(h, C.c_float(2.0), C.c_float(skirt)) == E_INVALID, skirt
    for r2 in (0.0, -1.0):  # a host table with r2 <= 0 in a real disc
        bad = table.copy()
        bad[2, 1, 2] = r2
        assert lib.mppi_set_discs(h, bad.ctypes.data_as(C.c_void_p), T, 3, 0, st) == E_INVALID
    reach, skirt = C.c_float(-1.0), C.c_float(-1.0)
    rig.h.call("mppi_get_disc_softness", C.byref(reach), C.byref(skirt))
    assert (reach.value, skirt.value) == (2.0, 1.0)
    same_bits("refused calls change nothing", rig.rollout(3), want)
    rig.close()
    hard = hard_rig(model, "n3", T, N)
    plain = plain_rig(model, "n3", T, N, hard.mean0)
    for other in (hard, plain):  # a hard or a plain handle: both new calls are another model's
        assert other.h.lib.mppi_set_disc_softness(other.h.h, C.c_float(2.0), C.c_float(0.5)) == E_INVALID
        assert other.h.lib.mppi_get_disc_softness(other.h.h, C.byref(reach), C.byref(skirt)) == E_INVALID
    bad = table.copy()
    bad[2, 1, 2] = 0.0
    hard.set_table(bad)  # the hard model takes r2 = 0 as before
    hard.close()
    plain.close()
    # the Python side: ValueError before anything reaches the library
    env = env_for(model, T)
    for pair in ((1.0, 0.5), (float("nan"), 0.5), (float("inf"), 0.5), (2.0, -0.1), (2.0, 1.1), (2.0, float("nan"))):
        with pytest.raises(ValueError):
            env.set_softness(*pair)
    with pytest.raises(ValueError):
        if model == "nav2d":
            env.set_moving_obstacles(torch.zeros(1, 2), torch.zeros(1, 2), 0.0)
        else:
            env.set_opponents([10], [1.0], 0.0)


# ------------------------------------------------------------------------------ 8. end to end through MPPI
@pytest.mark.parametrize("model", MODELS)
def test_tagged_against_untagged_end_to_end(model):
    """The tagged callables (fused) against the same callables behind plain lambdas (the generic path) on one injected noise
    block, disc weight 10 and lambda = 10 (a dense softmax), as the hard models' tests hold theirs.  Costs of both: the parity
    rule against float64 on that solve's own states.  action_seq of both: within 1e-5 of the float64 softmax over the device's
    own costs and clamped actions."""
    ref_mod = D if model == "nav2d" else RD
    T, N, lam, setting = 8, 1000 if model == "nav2d" else 512, 10.0, (2.0, 0.25)
    table, x0, ref = case(model, "n3", T)
    table = table.copy()
    table[:, :, 3] = 10.0
    env = env_for(model, T)
    env.set_softness(*setting)
    put_table(model, env, table)
    ab = R.coefficients(*setting)
    x = torch.from_numpy(f32(x0).copy()).cuda()
    rng = np.random.default_rng(9)
    eps = torch.from_numpy((ref_mod.MEAN + rng.standard_normal((N, T, 2)) * ref_mod.SIGMAS).astype(f32))
    for tag in (True, False):
        solver = solver_for(model, env, T, N, ref, tag=tag, lam=lam)
        solver.inject_noise(eps)
        a, s = solver.forward(x)
        c = solver._costs.cpu().numpy()
        U = solver._perturbed_action_seqs.cpu().numpy()
        S = solver._state_seq_batch.cpu().numpy()
        if model == "nav2d":
            P, grid = NAV.world(env)
            r64 = R.rollout_nav2d(P, grid, table, x0, U, ab[0], ab[1], f64, states=S)
        else:
            P, grids = RAC.world(solver._test_keep)
            r64 = R.rollout_racing(P, grids, ref, table, x0, U, ab[0], ab[1], f64, states=S)
        keep = ~(r64["near"] | r64["edge"])
        left = int(r64["near"].sum())
        err = np.abs(c.astype(f64) - r64["costs"])[keep].max() / r64["scale"]
        share = r64["skirted"].any(axis=(1, 2)).mean()
        print(f"[soft discs] {model} end to end tag={tag}: left out {left}, max err {err:.3g} of the scale, skirt share {share:.3f}")
        assert left <= R.cap(N) and err <= R.PARITY and share >= 0.05
        e, ess = weights64(c, lam)
        assert ess > 10.0  # dense, not an arg-min
        a64 = np.tensordot(e, U.astype(f64), axes=1) / e.sum()
        assert np.max(np.abs(a.cpu().numpy() - a64)) <= 1e-5, f"tag={tag}: action_seq {np.max(np.abs(a.cpu().numpy() - a64)):.3g}"


@pytest.mark.parametrize("model", MODELS)
def test_window_handles_equal_the_unsharded_handle(model):
    T, N, setting = 8, 200, (2.0, 0.25)
    whole = soft_rig(model, "n3", T, N, setting=setting, math=2)
    c = whole.rollout(5)
    whole.close()
    parts = []
    for off, n in ((0, 130), (130, 70)):
        w = soft_rig(model, "n3", T, n, setting=setting, math=2)
        w.window(off)  # (a new handle: _prepare hands the env's pair over again)
        w.h.call("mppi_set_option", b"math", 2)
        w.set_mean(w.mean0)
        parts.append(w.rollout(5))
        w.close()
    same_bits("two windows", np.concatenate(parts), c)


def test_deepcopy_continues_bit_identically_nav2d():
    from envs import SoftMovingObstacleNav2DEnv

    T, N = 8, 512
    env = SoftMovingObstacleNav2DEnv(horizon=T, soft_reach=3.0, soft_skirt=0.5)
    env.set_moving_obstacles([[-8.8, -8.6], [-8.5, -8.9]], [[0.2, -0.6], [-0.3, 0.5]], [0.25, 0.3], weight=10.0)
    solver = nav_solver(env, T, N, lam=10.0)
    x = env.reset().clone()
    for _ in range(2):
        a, s = solver.forward(x)
        x = s[0, 1].clone()
    twin = copy.deepcopy(solver)
    assert twin._cost_owner is not env and twin._h is not solver._h
    assert (twin._cost_owner.soft_reach, twin._cost_owner.soft_skirt) == (3.0, 0.5)
    for k in range(2):
        (a0, s0), (a1, s1) = solver.forward(x), twin.forward(x)
        same_bits(f"copy, solve {k}: action_seq", a1.cpu().numpy(), a0.cpu().numpy())
        same_bits(f"copy, solve {k}: costs", twin._costs.cpu().numpy(), solver._costs.cpu().numpy())
        x = s0[0, 1].clone()
    hard = copy.deepcopy(solver)
    hard._cost_owner.set_softness(2.0, 0.0)
    hard.forward(x)
    solver.forward(x)
    assert not np.array_equal(hard._costs.cpu().numpy(), solver._costs.cpu().numpy())  # (the pair matters in this scene)


def test_deepcopy_continues_bit_identically_racing():
    """Through the controller's own tick (the window built on the device, the cars' table padded on the device)"""
    from envs.racing_opponents import SoftOpponentRacingEnv, soft_opponent_racing_controller

    T, N = 8, 512
    env = SoftOpponentRacingEnv(horizon=T, soft_reach=3.0, soft_skirt=0.5)
    env.set_opponents([40, 70], [2.0, 1.0], [0.6, 0.5], lateral_offset=[0.3, -0.4], weight=10.0)
    ctrl = soft_opponent_racing_controller(env, horizon=T, num_samples=N, lambda_=10.0)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    x = env.reset().clone()
    x[3] = 4.0
    for _ in range(2):
        a, s = ctrl.update(x, env.racing_center_path)
        x = s[0, 1].clone()
    assert ctrl._window_on_device and ctrl.solver._model == "racing_discs_soft"
    solver = ctrl.solver
    twin = copy.deepcopy(solver)
    assert twin._cost_owner is not ctrl and twin._h is not solver._h
    for k in range(2):
        for sv in (solver, twin):
            sv.update_reference_window(x)
        (a0, s0), (a1, s1) = solver.forward(x), twin.forward(x)
        same_bits(f"copy, solve {k}: action_seq", a1.cpu().numpy(), a0.cpu().numpy())
        same_bits(f"copy, solve {k}: costs", twin._costs.cpu().numpy(), solver._costs.cpu().numpy())
        x = s0[0, 1].clone()
