"""Racing among moving discs (MPPI_MODEL_RACING_DISCS: envs/racing_opponents.py, mppi_set_discs) on a real MI355X.

Costs, states and clamped actions come from the C ABI's individual entry points (test_gpu_action_cost.Rig); the reference is
tests/racing_discs_ref.py on the EXPORTED actions, with the case table the CPU suite has already held to its claims.

  math 0    The cost arithmetic — subtract, multiply, add, divide, round, compare, the sequential fp32 sum — is exactly rounded
            everywhere, sin / cos / tan are not: the device's library and the host's differ in a last bit on some arguments, and
            one such bit moves a state.  So every sample's cost must equal, BIT FOR BIT, the fp32 restatement evaluated on the
            device's own state sequences (mppi_rollout_samples: the same strict functor), and those states must lie within
            5e-4 m of the restatement's own rollout: T <= 25 steps of two roundings of a position below 32 m (1.9e-6 each: 1e-4),
            plus a heading that drifts by a few ulp of pi per step (25 x 7e-7 rad) over a path of 10 m (2e-4).
  math 1, 2 the parity rule of DESIGN.md section 4 against the float64 restatement — 2e-6 of the cost scale — for every sample
            the boundary rule keeps (discs_ref: within 1e-4 m of a disc's edge, or 1e-3 cell of a map cell of another value);
            the number of samples left out at a disc's edge is printed and held to the cap max(2, 0.02 N).
  mapping 1 (a wavefront per trajectory) sums the stage costs by a wave reduction in fp32: the parity rule, at every level.
"""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import action_cost_ref as acref
import racing_discs_ref as R
from test_gpu_action_cost import LAM, Rig, measure, term
from test_gpu_covariance import _need_gpu, weights64
from test_gpu_fused_geometry import ALL_INHERIT, took

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
_envs = {}
E_INVALID, E_STATE = -1, -3


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(name, got, want):
    bad = int(np.sum(bits(got) != bits(want)))
    assert bad == 0, f"{name}: {bad} of {np.size(got)} values differ"


def env_for(T):
    _need_gpu()
    from envs.racing_opponents import OpponentRacingEnv

    if T not in _envs:
        _envs[T] = OpponentRacingEnv(horizon=T)
    return _envs[T]


def start_of(env):
    return f32(env.reset().cpu().numpy())


def case(name, T):
    """-> (table, x0, ref [T + 1, 4]): the window of the example's tick from the start pose"""
    env = env_for(T)
    table, x0 = R.case(name, T, start_of(env), float(env._obstacle_map.x_lim[1]))
    return table, x0, R.window(env.racing_center_path_np, start_of(env), T)


def put_table(env, table):
    """The case's table into the env's tensor (a new one: the set of cars changed), version bumped"""
    env._opp_table = torch.from_numpy(np.ascontiguousarray(table, f32)).cuda()
    env._opp_version += 1


def make_ctrl(env, T, N, ref, lam=1.0, **kw):
    from envs.racing_opponents import opponent_racing_controller

    ctrl = opponent_racing_controller(env, horizon=T, num_samples=N, lambda_=lam, **kw)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    ctrl.set_reference(ref)
    ctrl.solver._test_keep = ctrl
    assert ctrl.solver._model == "racing_discs"
    return ctrl


def make_untagged(env, T, N, ref, lam=1.0, **kw):
    """The same callables behind plain lambdas: the generic path"""
    from pi_mpc.mppi import MPPI

    ctrl = make_ctrl(env, T, 64, ref)
    solver = MPPI(horizon=T, num_samples=N, dim_state=4, dim_control=2, dynamics=lambda s, a: env.dynamics(s, a),
                  cost_func=lambda s, a, i: ctrl.cost_function(s, a, i), u_min=env.u_min, u_max=env.u_max,
                  sigmas=torch.tensor(R.SIGMAS), lambda_=lam, **kw)
    assert solver._model is None
    solver._test_keep = ctrl
    return solver


def world(ctrl):
    spec = type(ctrl).cost_function.__mppi_native__.provider(ctrl)
    grids = tuple((np.ascontiguousarray(g.cells, np.uint8), float(g.cell_size), float(g.origin[0]), float(g.origin[1]))
                  for g in spec["maps"])
    return f32(spec["params"]), grids


def states_of(rig):
    """[N, T + 1, 4]: every sample of the rig's last rollout re-rolled (mppi_rollout_samples)"""
    idx = torch.arange(rig.N, device="cuda", dtype=torch.int64)
    out = torch.empty(rig.N, rig.T + 1, 4, device="cuda")
    rig.h.call("mppi_rollout_samples", idx.data_ptr(), rig.N, out.data_ptr(), rig.solver._stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def plain_rig(T, N, x0, ref, mean, math=2, mode=None):
    """A plain racing handle: the parent classes' callables, the same maps, limits, reference window and seed"""
    from envs.racing_controller import racing_controller
    from envs.racing_env import RacingEnv

    plain = _envs.setdefault("plain", RacingEnv())
    ctrl = racing_controller(plain, horizon=T, num_samples=N, lambda_=1.0)
    ctrl.set_cost_map(plain._obstacle_map, plain._lane_map)
    ctrl.set_reference(ref)
    ctrl.solver._test_keep = ctrl
    assert ctrl.solver._model == "racing"
    b = Rig("racing", T, N, solver=(ctrl.solver, torch.from_numpy(f32(x0).copy())))
    b.ctrl = ctrl
    b.h.call("mppi_set_option", b"math", math)
    if mode is not None:
        b.h.call("mppi_set_option", b"fused_solve", mode)
    b.set_mean(mean)
    return b


class DiscRig(Rig):
    def __init__(self, table, x0, ref, T, N, math=0, mode=None, **kw):
        self.env = env_for(T)
        self.table = np.ascontiguousarray(table, f32)
        self.ref_path = np.ascontiguousarray(ref, f32)
        put_table(self.env, self.table)
        self.ctrl = make_ctrl(self.env, T, N, self.ref_path, **kw)
        self.P, self.grids = world(self.ctrl)
        super().__init__("racing_discs", T, N, solver=(self.ctrl.solver, torch.from_numpy(f32(x0).copy())))
        self.x0_host = f32(x0)
        self.h.call("mppi_set_option", b"math", math)
        if mode is not None:
            self.h.call("mppi_set_option", b"fused_solve", mode)
        self.mean0 = np.broadcast_to(R.MEAN, (T, 2)).copy()
        self.set_mean(self.mean0)

    def new_handle(self, offset=0, inherit=None, n=None):
        """A fresh handle of this model (Raw.window with racing's limits: helpers.MODEL_CFG does not know this model); nothing
        uploaded yet"""
        from mppi_playground_amd import _capi

        sol = self.solver
        cfg = _capi.MppiConfig()
        cfg.model = _capi.MODEL_IDS["racing_discs"]
        cfg.horizon, cfg.dim_state, cfg.dim_control = self.T, 4, 2
        cfg.num_samples, cfg.sample_offset = self.N if n is None else n, int(offset)
        cfg.inherit_count = ALL_INHERIT if inherit is None else int(inherit)
        for k in range(2):
            cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = float(R.U_MIN[k]), float(R.U_MAX[k]), float(R.SIGMAS[k])
        cfg.seed, cfg.device = sol._seed, 0
        sol._h.close()
        sol._h = _capi.Handle(cfg)
        sol._uploaded, sol._params_set, sol._ref_uploaded = {}, None, None

    def window(self, offset, inherit=None):
        self.new_handle(offset, inherit)
        self._prepare()

    def blank(self):
        """A fresh handle with parameters and maps only: neither part of the step table"""
        self.new_handle()
        sol = self.solver
        sol._h.discs_key = (id(sol._cost_owner), self.env._opp_version)  # (the solver believes the table is there)
        self.ctrl._window_on_device = True                               # (... and the window: nothing is uploaded)
        try:
            self._prepare()
        finally:
            self.ctrl._window_on_device = False
        self.set_mean(self.mean0)

    def set_table(self, table, on_device=False):
        st = self.solver._stream()
        t = np.ascontiguousarray(table, f32)
        if on_device:
            self._tab_dev = torch.from_numpy(t).cuda()
            self.h.call("mppi_set_discs", self._tab_dev.data_ptr(), t.shape[0], t.shape[1], 1, st)
        else:
            self.h.call("mppi_set_discs", t.ctypes.data_as(C.c_void_p) if t.size else None, t.shape[0], t.shape[1], 0, st)
        self.table = t

    def set_ref(self, ref):
        r = np.ascontiguousarray(ref, f32)
        self.h.call("mppi_set_reference", r.ctypes.data_as(C.c_void_p), r.shape[0], self.solver._stream())
        self.ref_path = r

    def get_ref(self, rows):
        out = torch.empty(rows, 4, device="cuda")
        self.h.call("mppi_get_reference", out.data_ptr(), rows, 1, self.solver._stream())
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def get_discs(self):
        rows, n = C.c_int(-1), C.c_int(-1)
        self.h.call("mppi_get_discs", None, C.byref(rows), C.byref(n), 1, self.solver._stream())
        out = torch.empty(rows.value, 8, 4, device="cuda")
        self.h.call("mppi_get_discs", out.data_ptr(), C.byref(rows), C.byref(n), 1, self.solver._stream())
        torch.cuda.synchronize()
        return out.cpu().numpy(), rows.value, n.value

    def states(self):
        return states_of(self)

    def ref(self, U, dtype=f32, **kw):
        return R.rollout(self.P, self.grids, self.ref_path, self.table, self.x0_host, U, dtype, **kw)


def rig_for(name, T, N, **kw):
    table, x0, ref = case(name, T)
    return DiscRig(table, x0, ref, T, N, **kw)


def check_level0(name, rig, c, U):
    S = rig.states()
    own = rig.ref(U, states=S)
    share = float(own["hit"].any(axis=(1, 2)).mean()) if own["hit"].size else 0.0
    if len(c) <= 128:  # (the all-numpy rollout calls the C library once per value: the small sample counts)
        free = rig.ref(U)
        dev = float(np.max(np.abs(S[..., :2].astype(f64) - free["S"][..., :2].astype(f64))))
        print(f"[racing discs] {name}: {int(np.sum(bits(c) == bits(free['costs'])))} of {len(c)} costs equal the all-numpy rollout "
              f"too; positions within {dev:.3g} of it; hit share {share:.3f}")
        assert dev <= 5e-4, f"{name}: positions {dev:.3g} from the restatement's rollout"
    else:
        print(f"[racing discs] {name}: hit share {share:.3f}")
    same_bits(f"{name}: costs against the fp32 restatement on the device's states", c, own["costs"])
    return own


def in_parity(name, rig, c, U):
    r64 = rig.ref(U, f64)
    left = int(r64["near"].sum())
    keep = ~(r64["near"] | r64["edge"])
    err = np.abs(c.astype(f64) - r64["costs"])
    worst = float(err[keep].max() / r64["scale"]) if keep.any() else 0.0
    print(f"[racing discs] {name}: left out {left} at a disc's edge (cap {R.cap(len(c))}), {int(r64['edge'].sum())} at a map cell's; "
          f"max err {worst:.3g} of the scale")
    assert np.all(np.isfinite(c)), name
    assert left <= R.cap(len(c)), f"{name}: the boundary rule leaves out {left} samples"
    assert worst <= R.PARITY, f"{name}: {worst:.3g} of the scale against {R.PARITY}"
    return r64


CASE_NAMES = list(R.CASES)
LONG = ("n8", "terminal", "pace")  # the cases that also run at T = 25


def shapes(name):
    """(T, N) of a case: every horizon at the ragged tile (the horizon decides which copies of the loop run), one tile and more
    than the single launch takes at the ragged and the complete last group (the sample count decides the launch path)"""
    return ([(T, 100) for T in R.HORIZONS if T < 25 or name in LONG]
            + [(T, N) for N in (R.SAMPLES[0], R.SAMPLES[2]) for T in (7, 8)])


# ------------------------------------------------------------------------------ 1. math 0: bit for bit
@pytest.mark.parametrize("name", CASE_NAMES)
def test_math0_costs_bit_for_bit(name):
    assert {N for _, N in shapes(name)} == set(R.SAMPLES)
    for T, N in shapes(name):
        rig = rig_for(name, T, N)
        tagname = f"{name} T{T} N{N}"
        c = rig.rollout(3)                        # the rollout kernel, noise regenerated in registers
        U = rig.actions_around(rig.mean0)
        own = check_level0(f"{tagname} regenerated", rig, c, U)
        rig.h.call("mppi_set_option", b"noise_regen", 0)
        same_bits(f"{tagname} tiles", rig.rollout(3), own["costs"])
        rig.h.call("mppi_set_option", b"noise_regen", 1)
        _, _, _, cs = rig.solve(3, LAM)           # mppi_solve: the single launch up to 4096 samples
        assert (took(rig.h) != (0, 0)) == (N <= 4096), tagname
        same_bits(f"{tagname} mppi_solve", cs, own["costs"])
        rig.close()


# ------------------------------------------------------------------------------ 2. the fast levels: the parity rule
@pytest.mark.parametrize("math", [1, 2])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_fast_levels_within_the_parity_rule(name, math):
    for T, N in shapes(name):
        rig = rig_for(name, T, N, math=math)
        tagname = f"{name} math {math} T{T} N{N}"
        c = rig.rollout(5)
        U = rig.actions_around(rig.mean0)
        in_parity(f"{tagname} regenerated", rig, c, U)
        rig.h.call("mppi_set_option", b"noise_regen", 0)
        in_parity(f"{tagname} tiles", rig, rig.rollout(5), U)
        rig.h.call("mppi_set_option", b"noise_regen", 1)
        if N <= 4096:
            _, _, _, c1 = rig.solve(5, LAM)
            assert took(rig.h) != (0, 0)
            in_parity(f"{tagname} single launch", rig, c1, U)
        rig.close()


@pytest.mark.parametrize("math", [0, 1, 2])
def test_wavefront_per_trajectory_mapping(math):
    rig = rig_for("n3", 8, 100, math=math)
    rig.h.call("mppi_set_option", b"mapping", 1)
    c = rig.rollout(6)
    in_parity(f"n3 math {math} mapping 1", rig, c, rig.actions_around(rig.mean0))
    rig.close()


# ------------------------------------------------------------------------------ 3. n = 0 against plain racing
@pytest.mark.parametrize("math", [0, 2])
@pytest.mark.parametrize("mode", [0, None])
def test_no_discs_equals_plain_racing(mode, math):
    """A handle with an empty table against a plain racing handle (the parent classes' callables, the same maps and window)
    on the same seed: costs, action_seq and state_seq bit-identical over three closed-loop solves.  T = 7 and 8: a ragged and
    a complete last group (the plain model walks its last group in the epilogue, this one in the loop)."""
    for T in (7, 8):
        N = 1000
        table, x0, ref = case("n0", T)
        a = DiscRig(table, x0, ref, T, N, math=math, mode=mode)
        b = plain_rig(T, N, x0, ref, a.mean0, math=math, mode=mode)
        x = f32(x0)
        for k in range(3):
            outs = []
            for rig in (a, b):
                rig.x0 = torch.from_numpy(x.copy()).cuda()
                rig.h.call("mppi_set_state", rig.x0.data_ptr(), 1, rig.solver._stream())
                outs.append(rig.solve(k + 1, 5.0))
                assert (took(rig.h) == (0, 0)) == (mode == 0)
            (aa, sa, _, ca), (ab, sb, _, cb) = outs
            same_bits(f"T{T} solve {k} costs", ca, cb)
            same_bits(f"T{T} solve {k} action_seq", aa, ab)
            same_bits(f"T{T} solve {k} state_seq", sa, sb)
            x = sa[1]
        a.close()
        b.close()


# ------------------------------------------------------------------------------ 4. every launch path on one mixed case
def test_every_launch_path_agrees():
    T, N = 8, 1000
    table, x0, ref = case("n3", T)
    mk = DiscRig(table, x0, ref, T, N, mode=0)
    a0, s0, _, c0 = mk.solve(4, 5.0)
    assert took(mk.h) == (0, 0)
    U = mk.actions_around(mk.mean0)
    own = check_level0("n3 multi-kernel", mk, c0, U)
    per_disc = own["hit"].any(1).mean(0)
    assert np.any((per_disc >= 0.05) & (per_disc <= 0.95)), per_disc  # both answers for some car
    sl = DiscRig(table, x0, ref, T, N)
    a1, s1, _, c1 = sl.solve(4, 5.0)
    assert took(sl.h) != (0, 0)
    same_bits("single launch costs", c1, c0)
    assert np.max(np.abs(a1 - a0)) <= 1e-5 and np.max(np.abs(s1 - s0)) <= 1e-4  # (another order of the weighted sums)
    # get_top_samples: the states of a PLAIN racing handle's samples on the same seed, in the order of THESE costs (the re-roll
    # is dynamics only: the cars change which samples are cheapest, not where a sample goes)
    plain = plain_rig(T, N, x0, ref, mk.mean0, math=0, mode=0)
    _, _, _, cp = plain.solve(4, 5.0)
    assert not np.array_equal(cp, c0)
    S_plain = states_of(plain)
    same_bits("re-rolled states: this model against plain racing", mk.states(), S_plain)
    k = 8
    st, w = torch.empty(k, T + 1, 4, device="cuda"), torch.empty(k, device="cuda")
    mk.h.call("mppi_top_samples", k, 5.0, st.data_ptr(), w.data_ptr(), mk.solver._stream())
    torch.cuda.synchronize()
    assert np.all(np.diff(w.cpu().numpy()) <= 0)
    order = np.argsort(c0, kind="stable")
    top = st.cpu().numpy()
    if len(np.unique(c0[order[:k + 1]])) == k + 1:  # no ties around the cut: the order is determined
        same_bits("top states", top, S_plain[order[:k]])
    else:
        cand = S_plain[c0 <= c0[order[k - 1]]]
        for row in top:
            assert any(np.array_equal(bits(row), bits(x)) for x in cand)
    plain.close()
    mk.close()
    sl.close()


def test_lazy_state_seq_through_forward():
    T, N = 8, 1000
    table, x0, ref = case("n3", T)
    env = env_for(T)
    put_table(env, table)
    outs = []
    for lazy in (False, True):
        solver = make_ctrl(env, T, N, ref, lam=5.0, lazy_state_seq=lazy).solver
        x = torch.from_numpy(f32(x0).copy()).cuda()
        seq = []
        for _ in range(3):
            a, s = solver.forward(x)
            seq.append((a.cpu().numpy().copy(), s.cpu().numpy().copy(), solver._costs.cpu().numpy().copy()))
            x = s[0, 1].clone()
        outs.append(seq)
    for (a0, s0, c0), (a1, s1, c1) in zip(*outs):
        same_bits("lazy costs", c1, c0)
        same_bits("lazy action_seq", a1, a0)
        same_bits("lazy state_seq", s1, s0)


def test_control_cost_instantiation_equals_the_separate_pass():
    T, N = 8, 200
    rig = rig_for("n3", T, N, math=2)
    mean = np.random.default_rng(7).uniform(R.U_MIN, R.U_MAX, (T, 2)).astype(f32)
    c0, c1, U, g = measure("racing_discs_in_rollout", rig, idx=7, mean=mean, sig=R.SIGMAS)
    term(rig, 0.0)
    assert np.array_equal(rig.rollout(7), c0)
    term(rig, 1.0)
    rig.h.call("mppi_add_action_cost", LAM, rig.solver._stream())
    added = rig.costs()
    acref.check("racing_discs_separate_pass", added, c0, acref.kappa32(1.0, LAM), g, U)
    same_bits("separate pass", added, c1)
    rig.close()


# ------------------------------------------------------------------------------ 5. one table, two writers
def _tick_windows(ctrl, env, states):
    """calc_ref_trajectory on the host for a sequence of states, the path index carried like the device's"""
    out, cind = [], 0
    for s in states:
        ref, cind = ctrl.calc_ref_trajectory(torch.from_numpy(s), env.racing_center_path, cind, ctrl.solver._horizon, DL=0.1,
                                             lookahead_distance=3, reference_path_interval=0.85)
        out.append(ref.numpy().copy())
    return out


def test_two_writers_in_either_order():
    """Discs first then the window, the window first then the discs, on handles that hold neither: each equals a handle given
    both afresh; a solve with one part only is refused; the getters return what was set."""
    T, N = 8, 1000
    t1, x0, ref1 = case("n3", T)
    t2, _, _ = case("overlap2", T)
    p0, h, _ = R._frame(x0)
    ref2 = R.window(env_for(T).racing_center_path_np, f32([p0[0] + 3.0 * h[0], p0[1] + 3.0 * h[1], 0, 0]), T)  # 3 m further on
    assert not np.array_equal(ref1, ref2)
    fresh = DiscRig(t2, x0, ref2, T, N, math=2)
    want = fresh.rollout(2)
    same_bits("get_reference of a fresh handle", fresh.get_ref(T + 1), ref2)
    fresh.close()
    other = DiscRig(t1, x0, ref2, T, N, math=2)
    assert not np.array_equal(other.rollout(2), want)
    other.close()
    for order in ("discs, window", "window, discs"):
        rig = DiscRig(t1, x0, ref1, T, N, math=2)
        rig.blank()
        lib, h, st = rig.h.lib, rig.h.h, rig.solver._stream()
        rig.h.call("mppi_sample", 2, st)
        assert lib.mppi_rollout_cost(h, st) == E_STATE                     # neither part
        if order == "discs, window":
            rig.set_table(t2)
            assert lib.mppi_rollout_cost(h, st) == E_STATE and b"reference" in lib.mppi_last_error(h)
            assert lib.mppi_solve(h, None, 2, C.c_float(1.0), rig.action.data_ptr(), rig.state.data_ptr(), rig.stats.data_ptr(), st) == E_STATE
            got, rows, n = rig.get_discs()                                 # (the discs can be read before the window is there)
            assert (rows, n) == (T, 2)
            rig.set_ref(ref2)
        else:
            rig.set_ref(ref2)
            assert lib.mppi_rollout_cost(h, st) == E_STATE and b"no disc table" in lib.mppi_last_error(h)
            assert lib.mppi_solve(h, None, 2, C.c_float(1.0), rig.action.data_ptr(), rig.state.data_ptr(), rig.stats.data_ptr(), st) == E_STATE
            same_bits("the window can be read before the discs are there", rig.get_ref(T + 1), ref2)
            rig.set_table(t2, on_device=True)
        same_bits(f"{order}: costs", rig.rollout(2), want)
        same_bits(f"{order}: window", rig.get_ref(T + 1), ref2)
        got, rows, n = rig.get_discs()
        assert (rows, n) == (T, 2)
        same_bits(f"{order}: padded discs", got, R.padded(t2))
        # each part rewritten without the other: the other part stays
        rig.set_ref(ref1)
        same_bits(f"{order}: discs after a new window", rig.get_discs()[0], R.padded(t2))
        rig.set_table(t1, on_device=order == "discs, window")
        same_bits(f"{order}: window after new discs", rig.get_ref(T + 1), ref1)
        again = DiscRig(t1, x0, ref1, T, N, math=2)
        same_bits(f"{order}: both rewritten", rig.rollout(2), again.rollout(2))
        again.close()
        rig.close()


def test_device_window_ticks_under_an_unchanged_disc_table():
    """mppi_ref_window rewrites floats 0-7 of every row for several ticks while the discs (floats 8-39) are written once: every
    tick's costs equal a handle given that tick's host-built window and the discs afresh.  A plain racing handle's
    mppi_ref_window output stays byte-identical to the host path's."""
    T, N = 8, 512
    table, x0, ref0 = case("n3", T)
    env = env_for(T)
    p0, h, _ = R._frame(x0)
    states = [f32([p0[0] + 0.8 * k * h[0], p0[1] + 0.8 * k * h[1], x0[2], x0[3]]) for k in range(4)]
    rig = DiscRig(table, x0, ref0, T, N, math=2)
    windows = _tick_windows(rig.ctrl, env, states)
    assert not np.array_equal(windows[0], windows[-1])
    plain = plain_rig(T, N, x0, ref0, rig.mean0)
    path = np.ascontiguousarray(env.racing_center_path_np, f32)
    dind = np.ascontiguousarray(rig.ctrl._window_offsets(T, 0.1, 3, 0.85), np.int32)
    for r in (rig, plain):
        r.h.call("mppi_set_center_path", path.ctypes.data_as(C.c_void_p), path.shape[0], dind.ctypes.data_as(C.c_void_p),
                 dind.shape[0], float(env.V_MAX))
    same_bits("set_center_path leaves the discs alone", rig.get_discs()[0], R.padded(table))
    for k, s in enumerate(states):
        sd = torch.from_numpy(s.copy()).cuda()
        for r in (rig, plain):
            r.h.call("mppi_set_state", sd.data_ptr(), 1, r.solver._stream())
            r.h.call("mppi_ref_window", sd.data_ptr(), r.solver._stream())
        same_bits(f"tick {k}: the window of this handle", rig.get_ref(T + 1), windows[k])
        out = torch.empty(T + 1, 4, device="cuda")
        plain.h.call("mppi_get_reference", out.data_ptr(), T + 1, 1, plain.solver._stream())
        torch.cuda.synchronize()
        same_bits(f"tick {k}: the window of a plain racing handle", out.cpu().numpy(), windows[k])
        same_bits(f"tick {k}: the discs", rig.get_discs()[0], R.padded(table))
        got = rig.rollout(k + 1)
        fresh = DiscRig(table, s, windows[k], T, N, math=2)
        same_bits(f"tick {k}: costs", got, fresh.rollout(k + 1))
        fresh.close()
    plain.close()
    rig.close()


# ------------------------------------------------------------------------------ 6. end to end through MPPI
def test_tagged_against_untagged_end_to_end():
    """The tagged callables (fused) against the same callables behind plain lambdas (the generic path) on one injected noise
    block at N = 512, T = 8, car weight 10 and lambda = 10 (a dense softmax).  Costs of both: the parity rule against the
    float64 restatement.  action_seq of both: within 1e-5 of the float64 softmax over the device's own costs and actions."""
    T, N, lam = 8, 512, 10.0
    table, x0, ref = case("n3", T)
    table = table.copy()
    table[:, :, 3] = 10.0
    env = env_for(T)
    put_table(env, table)
    x = torch.from_numpy(f32(x0).copy()).cuda()
    rng = np.random.default_rng(9)
    eps = torch.from_numpy((R.MEAN + rng.standard_normal((N, T, 2)) * R.SIGMAS).astype(f32))
    for tag in (True, False):
        solver = make_ctrl(env, T, N, ref, lam=lam).solver if tag else make_untagged(env, T, N, ref, lam=lam)
        P, grids = world(solver._test_keep)
        solver.inject_noise(eps)
        a, s = solver.forward(x)
        c = solver._costs.cpu().numpy()
        U = solver._perturbed_action_seqs.cpu().numpy()
        r64 = R.rollout(P, grids, ref, table, x0, U, f64)
        keep = ~(r64["near"] | r64["edge"])
        left = int(r64["near"].sum())
        err = np.abs(c.astype(f64) - r64["costs"])[keep].max() / r64["scale"]
        share = r64["hit"].any(axis=(1, 2)).mean()
        print(f"[racing discs] end to end tag={tag}: left out {left}, max err {err:.3g} of the scale, hit share {share:.3f}")
        assert left <= R.cap(N) and err <= R.PARITY
        e, ess = weights64(c, lam)
        assert ess > 10.0  # dense, not an arg-min
        a64 = np.tensordot(e, U.astype(f64), axes=1) / e.sum()
        assert np.max(np.abs(a.cpu().numpy() - a64)) <= 1e-5, f"tag={tag}: action_seq {np.max(np.abs(a.cpu().numpy() - a64)):.3g}"


# ------------------------------------------------------------------------------ 7. shard invariance
def test_window_handles_equal_the_unsharded_handle():
    T, N = 8, 200
    whole = rig_for("n3", T, N, math=2)
    c = whole.rollout(5)
    whole.close()
    parts = []
    for off, n in ((0, 130), (130, 70)):
        w = rig_for("n3", T, n, math=2)
        w.window(off)
        w.h.call("mppi_set_option", b"math", 2)
        w.set_mean(w.mean0)
        parts.append(w.rollout(5))
        w.close()
    same_bits("two windows", np.concatenate(parts), c)


def _shard_worker(rank, world_size, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["MPPI_EXCHANGE"] = "nccl"
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        import mppi_playground_amd  # noqa: F401

        a, s = _sharded_case(shard_samples=True)
        q.put((rank, a, s))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _sharded_case(**kw):
    T, N = 8, 1024
    table, x0, ref = case("n3", T)
    table = table.copy()
    table[:, :, 3] = 10.0
    env = env_for(T)
    put_table(env, table)
    solver = make_ctrl(env, T, N, ref, lam=10.0, **kw).solver
    a, s = solver.forward(torch.from_numpy(f32(x0).copy()).cuda())
    return a.cpu().numpy(), s.cpu().numpy()


def test_two_rank_sharded_solve_matches_the_unsharded_solve():
    """shard_samples=True with two ranks on this device (gloo; each rank uploads the same tables), as test_gpu_moving_discs.py
    measures the other disc model: the combine adds the two shard summaries in another order than the unsharded reduction, so
    the solve is held to 2e-6 of the largest entry, the two ranks to each other bit for bit."""
    _need_gpu()
    import socket

    import torch.multiprocessing as mp

    from helpers import rel_err

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
    a, s = _sharded_case()
    for r in res:
        assert rel_err(r[1], a) < 2e-6 and rel_err(r[2], s) < 2e-6
    same_bits("ranks: action_seq", res[0][1], res[1][1])
    same_bits("ranks: state_seq", res[0][2], res[1][2])


# ------------------------------------------------------------------------------ 8. deepcopy
def test_deepcopy_continues_bit_identically():
    """Through the controller's own tick (the window built on the device, the cars' table padded on the device): the copy
    carries both parts of the step table, the count and the path index."""
    from envs.racing_opponents import OpponentRacingEnv, opponent_racing_controller

    T, N = 8, 512
    env = OpponentRacingEnv(horizon=T)
    env.set_opponents([40, 70], [2.0, 1.0], [0.6, 0.5], lateral_offset=[0.3, -0.4], weight=10.0)
    ctrl = opponent_racing_controller(env, horizon=T, num_samples=N, lambda_=10.0)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    x = env.reset().clone()
    x[3] = 4.0
    for _ in range(2):
        a, s = ctrl.update(x, env.racing_center_path)
        x = s[0, 1].clone()
    assert ctrl._window_on_device
    solver = ctrl.solver
    twin = copy.deepcopy(solver)
    assert twin._cost_owner is not ctrl and twin._h is not solver._h
    for k in range(2):
        for sv in (solver, twin):  # the tick, by hand on both: window from the state, then the solve
            sv.update_reference_window(x)
        (a0, s0), (a1, s1) = solver.forward(x), twin.forward(x)
        same_bits(f"copy, solve {k}: action_seq", a1.cpu().numpy(), a0.cpu().numpy())
        same_bits(f"copy, solve {k}: costs", twin._costs.cpu().numpy(), solver._costs.cpu().numpy())
        same_bits(f"copy, solve {k}: window", twin.reference_window().cpu().numpy(), solver.reference_window().cpu().numpy())
        x = s0[0, 1].clone()
    assert twin.path_index == solver.path_index


# ------------------------------------------------------------------------------ 9. refusals
def test_refusals():
    T, N = 8, 64
    table, x0, ref = case("n3", T)
    rig = DiscRig(table, x0, ref, T, N)
    lib, h, st = rig.h.lib, rig.h.h, rig.solver._stream()
    nine = np.zeros((T, 9, 4), f32)
    assert lib.mppi_set_discs(h, nine.ctypes.data_as(C.c_void_p), T, 9, 0, st) == E_INVALID      # n = 9
    assert lib.mppi_set_discs(h, table.ctypes.data_as(C.c_void_p), 0, 3, 0, st) == E_INVALID     # rows < 1
    bad = table.copy()
    bad[2, 1, 0] = np.nan
    assert lib.mppi_set_discs(h, bad.ctypes.data_as(C.c_void_p), T, 3, 0, st) == E_INVALID       # a value that is not finite
    same_bits("refused tables change nothing", rig.rollout(3), rig_for("n3", T, N).rollout(3))
    rig.set_table(table[:T - 1])                                                                  # rows < T: refused at solve time
    rig.h.call("mppi_sample", 3, st)
    assert lib.mppi_rollout_cost(h, st) == E_STATE and b"fewer rows" in lib.mppi_last_error(h)
    assert lib.mppi_solve(h, None, 3, C.c_float(1.0), rig.action.data_ptr(), rig.state.data_ptr(), rig.stats.data_ptr(), st) == E_STATE
    rig.set_table(table)
    rig.set_ref(ref[:T - 1])                                                                      # a window shorter than the horizon
    assert lib.mppi_rollout_cost(h, st) == E_STATE and b"shorter than the horizon" in lib.mppi_last_error(h)
    rig.set_ref(ref)
    assert lib.mppi_rollout_cost(h, st) == 0
    plain = plain_rig(T, N, x0, ref, rig.mean0)
    pl, ph = plain.h.lib, plain.h.h
    assert pl.mppi_set_discs(ph, table.ctypes.data_as(C.c_void_p), T, 3, 0, st) == E_INVALID      # a plain racing handle
    assert pl.mppi_get_discs(ph, None, None, None, 0, st) == E_INVALID
    plain.close()
    rig.close()
    # the Python side: ValueError before anything reaches the library
    env = env_for(T)
    for wrong in (np.zeros((T, 9, 4), f32), np.zeros((T - 1, 2, 4), f32)):
        put_table(env, wrong)
        solver = make_ctrl(env, T, N, ref).solver
        with pytest.raises(ValueError):
            solver.forward(torch.from_numpy(f32(x0).copy()).cuda())
    put_table(env, table)


# ------------------------------------------------------------------------------ 10. the example's scenario, closed loop
def test_closed_loop_passes_the_cars_and_the_blind_solver_does_not():
    """example/racing_opponents.py at its own size (N = 4000, T = 25) for its own number of ticks — enough to reach and pass
    the three cars (the ego's path index ends beyond every car's).  With "racing_discs" no tick is in collision with a car; the
    same loop, same seed, same cars, driven by the plain "racing" solver collides: the scenario needs the feature."""
    _need_gpu()
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "example")
    if here not in sys.path:
        sys.path.insert(0, here)
    import racing_opponents as ex

    aware_hits, _, index = ex.run(ex.TICKS, opponent_aware=True)
    cars_end = [i + round(v * 0.1 * ex.TICKS / 0.1) for i, v in zip(ex.CARS["path_index"], ex.CARS["speed"])]
    assert index > max(cars_end), f"the ego ends at path index {index}, the cars at {cars_end}"
    assert aware_hits == 0
    blind_hits, _, _ = ex.run(ex.TICKS, opponent_aware=False)
    assert blind_hits >= 1
