"""The moving-disc model (MPPI_MODEL_NAV2D_DISCS: envs/navigation_2d_moving.py, mppi_set_discs) on a real MI355X.

Costs, states and clamped actions come from the C ABI's individual entry points (test_gpu_action_cost.Rig); the reference is
tests/discs_ref.py on the EXPORTED actions, with the case table the CPU suite has already held to its claims.

  math 0    The cost arithmetic — subtract, multiply, add, sqrt, divide, round, compare, the double accumulator — is exactly
            rounded everywhere, sin / cos are not: the device's library and the host's differ in a last bit on some arguments, and
            one such bit moves a state.  So every sample's cost must equal, BIT FOR BIT, the fp32 restatement evaluated on the
            device's own state sequences (mppi_rollout_samples: the same strict functor), and those states must lie within
            1e-4 m of the restatement's own rollout (T <= 25 steps of at most one ulp of a position below 10 m, 9.5e-7, plus the
            trig difference: 2.5e-5).  The count of costs that also equal the all-numpy rollout is printed, not asserted.
            Regenerated noise, materialised tiles, mppi_solve (the single launch up to 4096 samples) and the X0OUT copy.
  math 1, 2 the parity rule of DESIGN.md section 4 against the float64 restatement — 2e-6 of the cost scale — for every sample
            the boundary rule keeps (discs_ref: within 1e-4 m of a disc's edge, or 1e-3 cell of a map cell of another value);
            the number of samples left out at a disc's edge is printed and held to the cap max(2, 0.02 N).
  mapping 1 (a wavefront per trajectory) sums the stage costs by a wave reduction in fp32: the parity rule, at every level.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import action_cost_ref as acref
import discs_ref as R
from test_gpu_action_cost import LAM, Rig, measure, term
from test_gpu_covariance import _need_gpu, weights64
from test_gpu_fused_geometry import ALL_INHERIT, took

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
_envs = {}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(name, got, want):
    bad = int(np.sum(bits(got) != bits(want)))
    assert bad == 0, f"{name}: {bad} of {np.size(got)} values differ"


def env_for(T):
    _need_gpu()
    from envs import MovingObstacleNav2DEnv

    if T not in _envs:
        _envs[T] = MovingObstacleNav2DEnv(horizon=T)
    return _envs[T]


def world(env):
    m = env._obstacle_map.grid_spec()
    grid = (np.ascontiguousarray(m.cells, np.uint8), float(m.cell_size), float(m.origin[0]), float(m.origin[1]))
    return f32(type(env).cost_function.__mppi_native__.provider(env)["params"]), grid


def put_table(env, table):
    """The case's table into the env's tensor (a new one: the obstacle set changed), version bumped"""
    env._disc_table = torch.from_numpy(np.ascontiguousarray(table, f32)).cuda()
    env._disc_version += 1


def make_solver(env, T, N, lam=1.0, tag=True, **kw):
    from pi_mpc.mppi import MPPI

    dyn, cost = (env.dynamics, env.cost_function) if tag else ((lambda s, a: env.dynamics(s, a)), (lambda s, a, i: env.cost_function(s, a, i)))
    solver = MPPI(horizon=T, num_samples=N, dim_state=3, dim_control=2, dynamics=dyn, cost_func=cost, u_min=torch.tensor(R.U_MIN),
                  u_max=torch.tensor(R.U_MAX), sigmas=torch.tensor(R.SIGMAS), lambda_=lam, **kw)
    assert (solver._model == "nav2d_discs") if tag else (solver._model is None)
    return solver


def states_of(rig):
    """[N, T + 1, 3]: every sample of the rig's last rollout re-rolled (mppi_rollout_samples)"""
    idx = torch.arange(rig.N, device="cuda", dtype=torch.int64)
    out = torch.empty(rig.N, rig.T + 1, 3, device="cuda")
    rig.h.call("mppi_rollout_samples", idx.data_ptr(), rig.N, out.data_ptr(), rig.solver._stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def plain_rig(T, N, x0, mean, math=2, mode=None):
    """A plain nav2d handle: the parent class's callables, the same map, limits and seed"""
    from envs.navigation_2d import Navigation2DEnv
    from pi_mpc.mppi import MPPI

    plain = Navigation2DEnv()
    psolver = MPPI(horizon=T, num_samples=N, dim_state=3, dim_control=2, dynamics=plain.dynamics, cost_func=plain.cost_function,
                   u_min=torch.tensor(R.U_MIN), u_max=torch.tensor(R.U_MAX), sigmas=torch.tensor(R.SIGMAS), lambda_=1.0)
    assert psolver._model == "nav2d"
    b = Rig("nav2d", T, N, solver=(psolver, torch.from_numpy(f32(x0).copy())))
    b.h.call("mppi_set_option", b"math", math)
    if mode is not None:
        b.h.call("mppi_set_option", b"fused_solve", mode)
    b.set_mean(mean)
    return b


class DiscRig(Rig):
    def __init__(self, table, x0, T, N, math=0, mode=None, **kw):
        self.env = env_for(T)
        self.table = np.ascontiguousarray(table, f32)
        put_table(self.env, self.table)
        self.P, self.grid = world(self.env)
        super().__init__("nav2d_discs", T, N, solver=(make_solver(self.env, T, N, **kw), torch.from_numpy(f32(x0).copy())))
        self.x0_host = f32(x0)
        self.h.call("mppi_set_option", b"math", math)
        if mode is not None:
            self.h.call("mppi_set_option", b"fused_solve", mode)
        self.mean0 = np.broadcast_to(R.MEAN, (T, 2)).copy()
        self.set_mean(self.mean0)

    def window(self, offset, inherit=None):  # (Raw.window with nav2d's limits: helpers.MODEL_CFG does not know this model)
        from mppi_playground_amd import _capi

        sol = self.solver
        cfg = _capi.MppiConfig()
        cfg.model = _capi.MODEL_IDS["nav2d_discs"]
        cfg.horizon, cfg.dim_state, cfg.dim_control = self.T, 3, 2
        cfg.num_samples, cfg.sample_offset = self.N, int(offset)
        cfg.inherit_count = ALL_INHERIT if inherit is None else int(inherit)
        for k in range(2):
            cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = float(R.U_MIN[k]), float(R.U_MAX[k]), float(R.SIGMAS[k])
        cfg.seed, cfg.device = sol._seed, 0
        sol._h.close()
        sol._h = _capi.Handle(cfg)
        sol._uploaded, sol._params_set, sol._ref_uploaded = {}, None, None
        self._prepare()

    def set_table(self, table, on_device=False):
        st = self.solver._stream()
        t = np.ascontiguousarray(table, f32)
        if on_device:
            self._tab_dev = torch.from_numpy(t).cuda()
            self.h.call("mppi_set_discs", self._tab_dev.data_ptr(), t.shape[0], t.shape[1], 1, st)
        else:
            self.h.call("mppi_set_discs", t.ctypes.data_as(C.c_void_p), t.shape[0], t.shape[1], 0, st)
        self.table = t

    def states(self):
        return states_of(self)

    def ref(self, U, dtype=f32, **kw):
        return R.rollout(self.P, self.grid, self.table, self.x0_host, U, dtype, **kw)


def check_level0(name, rig, c, U):
    S = rig.states()
    own = rig.ref(U, states=S)
    free = rig.ref(U)
    dev = float(np.max(np.abs(S.astype(f64) - free["S"].astype(f64))))
    print(f"[discs] {name}: {int(np.sum(bits(c) == bits(free['costs'])))} of {len(c)} costs equal the all-numpy rollout too; "
          f"states within {dev:.3g} of it; hit share {float(own['hit'].any(axis=(1, 2)).mean()) if own['hit'].size else 0.0:.3f}")
    assert dev <= 1e-4, f"{name}: states {dev:.3g} from the restatement's rollout"
    same_bits(f"{name}: costs against the fp32 restatement on the device's states", c, own["costs"])
    return own


def in_parity(name, rig, c, U):
    r64 = rig.ref(U, f64)
    left = int(r64["near"].sum())
    keep = ~(r64["near"] | r64["edge"])
    err = np.abs(c.astype(f64) - r64["costs"])
    worst = float(err[keep].max() / r64["scale"]) if keep.any() else 0.0
    print(f"[discs] {name}: left out {left} at a disc's edge (cap {R.cap(len(c))}), {int(r64['edge'].sum())} at a map cell's; "
          f"max err {worst:.3g} of the scale")
    assert np.all(np.isfinite(c)), name
    assert left <= R.cap(len(c)), f"{name}: the boundary rule leaves out {left} samples"
    assert worst <= R.PARITY, f"{name}: {worst:.3g} of the scale against {R.PARITY}"
    return r64


CASE_NAMES = list(R.CASES)


# ------------------------------------------------------------------------------ 1. math 0: bit for bit
@pytest.mark.parametrize("name", CASE_NAMES)
def test_math0_costs_bit_for_bit(name):
    for T in R.HORIZONS + ((R.T_LONG,) if name in ("n8", "terminal") else ()):
        for N in R.SAMPLES:
            table, x0 = R.case(name, T)
            rig = DiscRig(table, x0, T, N)
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
    for T in R.HORIZONS + ((R.T_LONG,) if name in ("n8", "terminal") else ()):
        for N in R.SAMPLES:
            table, x0 = R.case(name, T)
            rig = DiscRig(table, x0, T, N, math=math)
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
    table, x0 = R.case("n3", 8)
    rig = DiscRig(table, x0, 8, 100, math=math)
    rig.h.call("mppi_set_option", b"mapping", 1)
    c = rig.rollout(6)
    in_parity(f"n3 math {math} mapping 1", rig, c, rig.actions_around(rig.mean0))
    rig.close()


# ------------------------------------------------------------------------------ 3. n = 0 against plain nav2d
@pytest.mark.parametrize("mode", [0, None])
def test_no_discs_equals_plain_nav2d(mode):
    """A handle with an empty table against a plain nav2d handle (the parent class's callables, the same map) on the same
    seed: costs, action_seq and state_seq bit-identical over three closed-loop solves, at the default math level."""
    T, N = 8, 1000
    table, x0 = R.case("n0", T)
    a = DiscRig(table, x0, T, N, math=2, mode=mode)
    b = plain_rig(T, N, x0, a.mean0, math=2, mode=mode)
    x = f32(x0)
    for k in range(3):
        outs = []
        for rig in (a, b):
            rig.x0 = torch.from_numpy(x.copy()).cuda()
            rig.h.call("mppi_set_state", rig.x0.data_ptr(), 1, rig.solver._stream())
            outs.append(rig.solve(k + 1, 5.0))
            assert (took(rig.h) == (0, 0)) == (mode == 0)
        (aa, sa, _, ca), (ab, sb, _, cb) = outs
        same_bits(f"solve {k} costs", ca, cb)
        same_bits(f"solve {k} action_seq", aa, ab)
        same_bits(f"solve {k} state_seq", sa, sb)
        x = sa[1]
    a.close()
    b.close()


# ------------------------------------------------------------------------------ 4. every launch path on one mixed case
def test_every_launch_path_agrees():
    T, N = 8, 1000
    table, x0 = R.case("n3", T)
    mk = DiscRig(table, x0, T, N, mode=0)
    a0, s0, _, c0 = mk.solve(4, 5.0)
    assert took(mk.h) == (0, 0)
    U = mk.actions_around(mk.mean0)
    own = check_level0("n3 multi-kernel", mk, c0, U)
    assert 0.05 <= own["hit"].any(axis=(1, 2)).mean() <= 0.95
    sl = DiscRig(table, x0, T, N)
    a1, s1, _, c1 = sl.solve(4, 5.0)
    assert took(sl.h) != (0, 0)
    same_bits("single launch costs", c1, c0)
    assert np.max(np.abs(a1 - a0)) <= 1e-5 and np.max(np.abs(s1 - s0)) <= 1e-5  # (another order of the weighted sums)
    # get_top_samples: the states of a PLAIN nav2d handle's samples on the same seed, in the order of THESE costs (the re-roll
    # is dynamics only: the discs change which samples are cheapest, not where a sample goes)
    plain = plain_rig(T, N, x0, mk.mean0, math=0, mode=0)
    plain.solve(4, 5.0)
    S_plain = states_of(plain)
    same_bits("re-rolled states: this model against plain nav2d", mk.states(), S_plain)
    k = 8
    st, w = torch.empty(k, T + 1, 3, device="cuda"), torch.empty(k, device="cuda")
    mk.h.call("mppi_top_samples", k, 5.0, st.data_ptr(), w.data_ptr(), mk.solver._stream())
    torch.cuda.synchronize()
    assert np.all(np.diff(w.cpu().numpy()) <= 0)
    order = np.argsort(c0, kind="stable")
    top = st.cpu().numpy()
    if len(np.unique(c0[order[:k + 1]])) == k + 1:  # no ties around the cut: the order is determined
        same_bits("top states", top, S_plain[order[:k]])
    else:  # (samples whose speed was clamped to 0 throughout share one trajectory and one cost)
        cand = S_plain[c0 <= c0[order[k - 1]]]
        for row in top:
            assert any(np.array_equal(bits(row), bits(x)) for x in cand)
    plain.close()
    mk.close()
    sl.close()


def test_lazy_state_seq_through_forward():
    T, N = 8, 1000
    table, x0 = R.case("n3", T)
    env = env_for(T)
    put_table(env, table)
    outs = []
    for lazy in (False, True):
        solver = make_solver(env, T, N, lam=5.0, lazy_state_seq=lazy)
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
    table, x0 = R.case("n3", T)
    rig = DiscRig(table, x0, T, N, math=2)
    mean = np.random.default_rng(7).uniform(R.U_MIN, R.U_MAX, (T, 2)).astype(f32)
    c0, c1, U, g = measure("nav2d_discs_in_rollout", rig, idx=7, mean=mean, sig=R.SIGMAS)
    term(rig, 0.0)
    assert np.array_equal(rig.rollout(7), c0)
    term(rig, 1.0)
    rig.h.call("mppi_add_action_cost", LAM, rig.solver._stream())
    added = rig.costs()
    acref.check("nav2d_discs_separate_pass", added, c0, acref.kappa32(1.0, LAM), g, U)
    same_bits("separate pass", added, c1)
    rig.close()


def test_graph_callables_follow_the_table_in_place():
    """The untagged callables captured into a graph (graph_callables=True) against the same callables run eagerly: the table is
    one tensor updated in place, so the replayed graph reads each tick's prediction."""
    T, N = 8, 256
    from envs import MovingObstacleNav2DEnv

    outs = []
    for graph in (False, True):
        env = MovingObstacleNav2DEnv(horizon=T)
        env.set_moving_obstacles([[-8.8, -8.6], [-8.5, -8.9]], [[0.2, -0.6], [-0.3, 0.5]], [0.25, 0.3], weight=10.0)
        solver = make_solver(env, T, N, lam=10.0, tag=False, graph_callables=graph)
        x = env.reset().clone()
        seq = []
        for _ in range(4):  # warm-up, capture, two replays
            a, s = solver.forward(x)
            seq.append((a.cpu().numpy().copy(), solver._costs.cpu().numpy().copy()))
            x, _ = env.step(a[0])
            x = x.clone()
        outs.append(seq)
    for k, ((a0, c0), (a1, c1)) in enumerate(zip(*outs)):
        same_bits(f"tick {k} costs", c1, c0)
        same_bits(f"tick {k} action_seq", a1, a0)


# ------------------------------------------------------------------------------ 5. the table's hand-over
def test_table_handover_in_stream_order():
    T, N = 8, 1000
    t1, x0 = R.case("n3", T)
    t2, _ = R.case("weights8", T)
    got = {}
    for how in ("host", "device"):
        rig = DiscRig(t1, x0, T, N, math=2)
        rig.solve(1, 5.0)
        rig.set_mean(rig.mean0)
        rig.set_table(t2, on_device=how == "device")
        _, _, _, got[how] = rig.solve(2, 5.0)
        rows, n = C.c_int(-1), C.c_int(-1)
        out = torch.empty(T, 8, 4, device="cuda")
        rig.h.call("mppi_get_discs", out.data_ptr(), C.byref(rows), C.byref(n), 1, rig.solver._stream())
        torch.cuda.synchronize()
        assert (rows.value, n.value) == (T, 8)
        same_bits(f"{how}: padded table", out.cpu().numpy(), R.padded(t2))
        host = np.empty((T, 8, 4), f32)
        rig.set_table(t1[:, :2])
        rig.h.call("mppi_get_discs", host.ctypes.data_as(C.c_void_p), C.byref(rows), C.byref(n), 0, rig.solver._stream())
        assert (rows.value, n.value) == (T, 2)
        same_bits(f"{how}: padded table to the host", host, R.padded(t1[:, :2]))
        rig.close()
    fresh = DiscRig(t2, x0, T, N, math=2)
    _, _, _, want = fresh.solve(2, 5.0)
    fresh.close()
    same_bits("host table, second solve", got["host"], want)
    same_bits("device table, second solve", got["device"], want)
    other = DiscRig(t1, x0, T, N, math=2)
    assert not np.array_equal(want, other.solve(2, 5.0)[3])
    other.close()


# ------------------------------------------------------------------------------ 6. end to end through MPPI
def test_tagged_against_untagged_end_to_end():
    """The env's tagged callables (fused) against the same callables behind plain lambdas (the generic path) on one injected
    noise block, disc weight 10 and lambda = 10 (a dense softmax).  Costs of both: the parity rule against the float64
    restatement.  action_seq of both: within 1e-5 of the float64 softmax over the device's own costs and clamped actions."""
    from envs import MovingObstacleNav2DEnv

    T, N, lam = 8, 1000, 10.0
    env = MovingObstacleNav2DEnv(horizon=T)
    table, x0 = R.case("n3", T)
    table = table.copy()
    table[:, :, 3] = 10.0
    put_table(env, table)
    P, grid = world(env)
    x = torch.from_numpy(f32(x0).copy()).cuda()
    rng = np.random.default_rng(9)
    # (first solve: zero warm start.  The injected block carries the mean action itself, so U = clamp(0 + eps) is spread
    # around v = 1 m/s like the table's placements expect)
    eps = torch.from_numpy((R.MEAN + rng.standard_normal((N, T, 2)) * R.SIGMAS).astype(f32))
    for tag in (True, False):
        solver = make_solver(env, T, N, lam=lam, tag=tag)
        solver.inject_noise(eps)
        a, s = solver.forward(x)
        c = solver._costs.cpu().numpy()
        U = solver._perturbed_action_seqs.cpu().numpy()
        r64 = R.rollout(P, grid, table, x0, U, f64)
        keep = ~(r64["near"] | r64["edge"])
        left = int(r64["near"].sum())
        err = np.abs(c.astype(f64) - r64["costs"])[keep].max() / r64["scale"]
        share = r64["hit"].any(axis=(1, 2)).mean()
        print(f"[discs] end to end tag={tag}: left out {left}, max err {err:.3g} of the scale, hit share {share:.3f}")
        assert left <= R.cap(N) and err <= R.PARITY
        e, ess = weights64(c, lam)
        assert ess > 20.0  # dense, not an arg-min
        a64 = np.tensordot(e, U.astype(f64), axes=1) / e.sum()
        assert np.max(np.abs(a.cpu().numpy() - a64)) <= 1e-5, f"tag={tag}: action_seq {np.max(np.abs(a.cpu().numpy() - a64)):.3g}"


# ------------------------------------------------------------------------------ 7. shard invariance
def test_window_handles_equal_the_unsharded_handle():
    T, N = 8, 200
    table, x0 = R.case("n3", T)
    whole = DiscRig(table, x0, T, N, math=2)
    c = whole.rollout(5)
    whole.close()
    parts = []
    for off, n in ((0, 130), (130, 70)):
        w = DiscRig(table, x0, T, n, math=2)
        w.window(off)
        w.h.call("mppi_set_option", b"math", 2)
        w.set_mean(w.mean0)
        parts.append(w.rollout(5))
        w.close()
    same_bits("two windows", np.concatenate(parts), c)


def _shard_worker(rank, world, port, q):
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["MPPI_EXCHANGE"] = "nccl"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import mppi_playground_amd  # noqa: F401

        a, s = _sharded_case(shard_samples=True)
        q.put((rank, a, s))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _sharded_case(**kw):
    T, N = 8, 1024
    table, x0 = R.case("n3", T)
    table = table.copy()
    table[:, :, 3] = 10.0
    env = env_for(T)
    put_table(env, table)
    solver = make_solver(env, T, N, lam=10.0, **kw)
    solver._h.call("mppi_set_mean", torch.from_numpy(np.broadcast_to(R.MEAN, (T, 2)).copy()).cuda().data_ptr(), 1, solver._stream())
    a, s = solver.forward(torch.from_numpy(f32(x0).copy()).cuda())
    return a.cpu().numpy(), s.cpu().numpy()


def test_two_rank_sharded_solve_matches_the_unsharded_solve():
    """shard_samples=True with two ranks on this device (gloo; each rank uploads the same table), as tests/test_gpu_parity.py
    and test_gpu_mlp_model.py measure the other models: the combine adds the two shard summaries in another order than the
    unsharded reduction, so the solve is held to 2e-6 of the largest entry, the two ranks to each other bit for bit.  (The
    per-sample costs of window handles are bit-identical: the test above.)"""
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
    T, N = 8, 512
    from envs import MovingObstacleNav2DEnv

    env = MovingObstacleNav2DEnv(horizon=T)
    env.set_moving_obstacles([[-8.8, -8.6], [-8.5, -8.9]], [[0.2, -0.6], [-0.3, 0.5]], [0.25, 0.3], weight=10.0)
    solver = make_solver(env, T, N, lam=10.0)
    x = env.reset().clone()
    for _ in range(2):
        a, s = solver.forward(x)
        x = s[0, 1].clone()
    twin = copy.deepcopy(solver)
    assert twin._cost_owner is not env and twin._h is not solver._h
    for k in range(2):
        (a0, s0), (a1, s1) = solver.forward(x), twin.forward(x)
        same_bits(f"copy, solve {k}: action_seq", a1.cpu().numpy(), a0.cpu().numpy())
        same_bits(f"copy, solve {k}: costs", twin._costs.cpu().numpy(), solver._costs.cpu().numpy())
        x = s0[0, 1].clone()


# ------------------------------------------------------------------------------ 9. refusals
def test_refusals():
    from mppi_playground_amd._capi import MppiError

    T, N = 8, 64
    table, x0 = R.case("n3", T)
    rig = DiscRig(table, x0, T, N)
    lib, h, st = rig.h.lib, rig.h.h, rig.solver._stream()
    nine = np.zeros((T, 9, 4), f32)
    assert lib.mppi_set_discs(h, nine.ctypes.data_as(C.c_void_p), T, 9, 0, st) == -1      # n = 9
    assert lib.mppi_set_discs(h, table.ctypes.data_as(C.c_void_p), 0, 3, 0, st) == -1     # rows < 1
    bad = table.copy()
    bad[2, 1, 0] = np.nan
    assert lib.mppi_set_discs(h, bad.ctypes.data_as(C.c_void_p), T, 3, 0, st) == -1       # a value that is not finite
    bad = table.copy()
    bad[0, 0, 3] = -1.0
    assert lib.mppi_set_discs(h, bad.ctypes.data_as(C.c_void_p), T, 3, 0, st) == -1       # a negative penalty
    same_bits("refused tables change nothing", rig.rollout(3), DiscRig(table, x0, T, N).rollout(3))
    rig.set_table(table[:T - 1])                                                           # rows < T: refused at solve time
    rig.h.call("mppi_sample", 3, st)
    assert lib.mppi_rollout_cost(h, st) == -3 and b"fewer rows" in lib.mppi_last_error(h)
    assert lib.mppi_solve(h, None, 3, C.c_float(1.0), rig.action.data_ptr(), rig.state.data_ptr(), rig.stats.data_ptr(), st) == -3
    # a horizon whose table rows do not fit in LDS next to the mean groups: refused by name, not as a failed launch
    long_T = 1400  # (128 B per row: 179 KB, more than the 160 KB of LDS a gfx950 block can have)
    far = np.broadcast_to(R.FAR, (long_T, 1, 4)).copy()
    big = DiscRig(far, x0, long_T, N)
    big.h.call("mppi_sample", 3, st)
    assert big.h.lib.mppi_rollout_cost(big.h.h, st) == -1 and b"do not fit in LDS" in big.h.lib.mppi_last_error(big.h.h)
    big.close()
    _envs.pop(long_T, None)
    # before any table: a new handle with parameters and map, the table's upload skipped
    rig.window(0)
    sol = rig.solver
    plain = Rig("nav2d", T, N)
    assert plain.h.lib.mppi_set_discs(plain.h.h, table.ctypes.data_as(C.c_void_p), T, 3, 0, st) == -1  # another model's handle
    plain.close()
    from mppi_playground_amd import _capi

    cfg = _capi.MppiConfig()
    cfg.model, cfg.horizon, cfg.dim_state, cfg.dim_control, cfg.num_samples = 9, T, 3, 2, N
    cfg.inherit_count, cfg.seed = ALL_INHERIT, 1
    for k in range(2):
        cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = float(R.U_MIN[k]), float(R.U_MAX[k]), float(R.SIGMAS[k])
    sol._h.close()
    sol._h = _capi.Handle(cfg)
    sol._uploaded, sol._params_set = {}, None
    sol._h.discs_key = (id(sol._cost_owner), rig.env._disc_version)  # (the solver believes the table is there: not uploaded)
    sol._refresh_model_inputs()
    sol._h.call("mppi_sample", 3, st)
    with pytest.raises(MppiError, match="no disc table"):
        sol._h.call("mppi_rollout_cost", st)
    sol._h.close()
    # the Python side: ValueError before anything reaches the library
    env = env_for(T)
    for wrong in (np.zeros((T, 9, 4), f32), np.zeros((T - 1, 2, 4), f32)):
        put_table(env, wrong)
        solver = make_solver(env, T, N)
        with pytest.raises(ValueError):
            solver.forward(torch.from_numpy(f32(x0).copy()).cuda())
    put_table(env, table)
