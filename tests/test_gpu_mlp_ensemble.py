"""Model ensembles for the learned dynamics (envs.MLPEnsemble; mppi_set_mlp_ensemble, mppi_set_particle_members) on a real
MI355X: one particle per network.

The solver is its own oracle, as in tests/test_gpu_particles.py: row m of the [P, N] matrix must equal what a PLAIN handle
holding member members[m]'s table (mppi_set_mlp) computes from x0 = particles[m] with the same seed, solve index and mean —
bit for bit at math level 0.  At the fast levels the functor is inlined into another kernel and contraction may differ: every
row is held to the rule tests/test_gpu_mlp_model.py applies to the plain kernel (mlp_ref.band: 4 x the distance of the fp32
restatement from float64 on the same actions, floored at 2 * 2^-24 * sum |cost terms|), and the number of bit-equal entries is
printed.  Everything outside the particle rollout is the NOMINAL member's.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import action_cost_ref as acref
import mlp_ensemble_cases as EC
import mlp_ref as R
from pi_mpc import _host
from test_gpu_action_cost import Rig, term
from test_gpu_covariance import _need_gpu
from test_gpu_fused_geometry import took
from test_gpu_particles import costs_of, matrix_of, min_of, put_particles, risk, same_bits, set_state, stream

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
LAM = 2.0


# ------------------------------------------------------------------------------ solvers and handles
def common(cs, T, N, lam):
    return dict(horizon=T, num_samples=N, dim_state=4, dim_control=cs["dc"], u_min=torch.tensor(cs["u_min"]),
                u_max=torch.tensor(cs["u_max"]), sigmas=torch.tensor(cs["sigmas"]), lambda_=lam)


def ens_solver(cs, T, N, nominal=0, lam=LAM, **kw):
    _need_gpu()
    from envs import MLPEnsemble
    from pi_mpc.mppi import MPPI

    ens = MLPEnsemble(EC.models(cs), nominal=nominal)
    solver = MPPI(dynamics=ens.dynamics, cost_func=ens.cost, **common(cs, T, N, lam), **kw)
    assert solver._model == cs["model"]
    return solver, ens


def member_solver(cs, e, T, N, lam=LAM, **kw):
    _need_gpu()
    from pi_mpc.mppi import MPPI

    model = EC.models(cs)[e]
    solver = MPPI(dynamics=model.dynamics, cost_func=model.cost, **common(cs, T, N, lam), **kw)
    assert solver._model == cs["model"]
    return solver, model


class ERig(Rig):
    """test_gpu_action_cost.Rig around an ensemble (member=None) or around ONE member as a plain MLPModel handle."""

    def __init__(self, cs, T, N, math=0, nominal=0, member=None, **kw):
        self.cs = cs
        if member is None:
            solver, self.ens = ens_solver(cs, T, N, nominal, **kw)
        else:
            solver, self.mlp = member_solver(cs, member, T, N, **kw)
        super().__init__(cs["model"], T, N, solver=(solver, torch.from_numpy(R.X0.copy())))
        self.math = math
        self.h.call("mppi_set_option", b"math", math)
        self.h.call("mppi_set_option", b"fused_solve", 0)

    def put_table(self, table):
        """(plain handles) another member's table, through mppi_set_mlp"""
        cs = self.cs
        t = np.ascontiguousarray(table, f32)
        self.h.call("mppi_set_mlp", t.ctypes.data_as(C.c_void_p), int(t.size), cs["hidden_layers"], int(cs["activation"] == "tanh"),
                    int(cs["residual"]), stream())

    def members(self, members):
        if members is None:
            self.h.call("mppi_set_particle_members", None, 0)
        else:
            self.h.call("mppi_set_particle_members", (C.c_int * len(members))(*members), len(members))

    def window(self, offset):
        """Re-create the handle as the N samples from global index `offset` on (Raw.window, with this case's limits)."""
        from mppi_playground_amd import _capi

        sol, cs = self.solver, self.cs
        cfg = _capi.MppiConfig()
        cfg.model = _capi.MODEL_IDS[cs["model"]]
        cfg.horizon, cfg.dim_state, cfg.dim_control = self.T, 4, cs["dc"]
        cfg.num_samples, cfg.sample_offset, cfg.inherit_count = self.N, int(offset), 1 << 40
        for k in range(cs["dc"]):
            cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = cs["u_min"][k], cs["u_max"][k], cs["sigmas"][k]
        cfg.seed, cfg.device = sol._seed, 0
        sol._h.close()
        sol._h = _capi.Handle(cfg)
        sol._uploaded, sol._params_set, sol._ref_uploaded = {}, None, None
        self._prepare()
        self.h.call("mppi_set_option", b"math", self.math)  # (a new handle starts at the default level)
        self.h.call("mppi_set_option", b"fused_solve", 0)

    def states_of(self, actions):
        """mppi_rollout_actions of one action sequence from the handle's state -> [T + 1, 4]"""
        a = torch.from_numpy(np.ascontiguousarray(actions, f32)).cuda()
        out = torch.full((1, self.T + 1, 4), float("nan"), device="cuda")
        self.h.call("mppi_rollout_actions", a.data_ptr(), 1, None, out.data_ptr(), stream())
        torch.cuda.synchronize()
        return out.cpu().numpy()[0]

    def top_states(self, k, lam):
        st, w = torch.empty(k, self.T + 1, 4, device="cuda"), torch.empty(k, device="cuda")
        self.h.call("mppi_top_samples", k, float(lam), st.data_ptr(), w.data_ptr(), stream())
        torch.cuda.synchronize()
        return st.cpu().numpy()


def a_mean(cs, T, seed):
    rng = np.random.default_rng(seed)
    return (0.3 * rng.uniform(f32(cs["u_min"]), f32(cs["u_max"]), (T, cs["dc"]))).astype(f32)


def plain_rows(b, tables, members, parts, idx):
    """[P, N]: the plain handle's costs of solve `idx` with member members[m]'s table from particles[m]"""
    rows = []
    for e, x in zip(members, parts):
        b.put_table(tables[e])
        set_state(b, x)
        rows.append(b.rollout(idx))
    return np.stack(rows)


def particle_rows(a, parts, members, idx, on_device=False):
    put_particles(a.h, parts, on_device)
    a.members(members)
    c = a.rollout(idx)
    return matrix_of(a.h, len(parts), a.N), c


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def rows_in_band(name, a, M, tables, members, parts, mean):
    """Every row against the float64 restatement through ITS member from ITS particle: mlp_ref.band, as test_gpu_mlp_model.in_band"""
    cs = a.cs
    U = a.actions_around(mean)
    for m, (e, x) in enumerate(zip(members, parts)):
        c32, _, mag = EC.ref(cs, e, x, U, table=tables[e])
        c64, _, _ = EC.ref(cs, e, x, U, f64, table=tables[e])
        limit, yard = R.band(c32, c64, mag)
        err = np.abs(M[m].astype(f64) - c64)
        print(f"[ensemble] {name} particle {m} (member {e}): ratio {err.max() / max(yard, 1e-300):.2f} of the fp32 band {yard:.3g}")
        assert np.all(np.isfinite(M[m])), name
        assert np.all(err <= limit), f"{name} particle {m}: {int((err > limit).sum())} costs beyond the band, worst {err.max():.3g}"


def check_rows(name, a, b, tables, members, parts, idx, mean, math, fold=("mean", 1)):
    mats = []
    for regen in (1, 0):
        for r in (a, b):
            r.h.call("mppi_set_option", b"noise_regen", regen)
        risk(a.h, *fold)
        M, c = particle_rows(a, parts, members, idx, on_device=bool(regen))
        want = plain_rows(b, tables, members, parts, idx)
        assert np.all(np.isfinite(M)), name
        if math == 0:
            for m in range(len(parts)):
                same_bits(f"{name} regen={regen} particle {m} (member {members[m]})", M[m], want[m])
        else:
            eq = int(np.sum(bits(M) == bits(want)))
            print(f"[ensemble] {name} math {math} regen={regen}: {eq} of {M.size} values equal the plain kernel's bit for bit")
            rows_in_band(f"{name} math {math} regen={regen}", a, M, tables, members, parts, mean)
        same_bits(f"{name} regen={regen}: folded", c, _host.fold_particle_costs(M, *fold))
        same_bits(f"{name} regen={regen}: minimum", [min_of(a.h)], [c.min()])
        mats.append(M)
    if math == 0:
        same_bits(f"{name}: regenerated noise against tiles", mats[0], mats[1])
    return mats[1]  # (the handles are left reading tiles)


# ------------------------------------------------------------------------------ 1. rows against plain handles
@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(EC.ARCHS))
def test_rows_equal_plain_handles_holding_the_members_tables(name, math):
    cs = EC.case(name)
    members = list(EC.MEMBERS)
    for T in EC.HORIZONS:
        for N in EC.SIZES_N:
            a, b = ERig(cs, T, N, math=math), ERig(cs, T, N, math=math, member=0)
            mean = a_mean(cs, T, T + N)
            a.set_mean(mean), b.set_mean(mean)
            M = check_rows(f"{name} T={T} N={N}", a, b, cs["tables"], members, EC.PARTS, 3, mean, math, ("cvar", 2))
            # particles 0 and 4 share member 0, particles 0 and 3 differ in member AND state: the rows are not one row
            assert not np.array_equal(M[0], M[4]) and not np.array_equal(M[0], M[3])
            # the same particles without a map all go through the nominal member
            Mn, _ = particle_rows(a, EC.PARTS, None, 3)
            if math == 0:
                same_bits("no map: nominal member", Mn, plain_rows(b, cs["tables"], [0] * EC.P, EC.PARTS, 3))
            assert not np.array_equal(Mn[0], M[0]) and np.array_equal(Mn[1], M[1])
            a.close(), b.close()


# ------------------------------------------------------------------------------ 2. the feature off is today's code path
@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp42_tanh_1l_abs"])
def test_ensemble_of_one_without_members_is_the_plain_model(name):
    cs = EC.case(name, 1)
    T, N = 8, 300
    for parts in (None, torch.from_numpy(EC.PARTS).cuda()):
        one, _ = ens_solver(cs, T, N, risk="cvar", risk_alpha=0.5)
        plain, _ = member_solver(cs, 0, T, N, risk="cvar", risk_alpha=0.5)
        x0 = torch.from_numpy(R.X0.copy()).cuda()
        for tick in range(3):
            outs = []
            for s in (one, plain):
                if parts is not None:
                    s.set_state_particles(parts)
                a, st = s.forward(x0)
                outs.append((a, st, s._costs, s.particle_costs if parts is not None else None))
            assert one.particle_members is None
            for got, want, what in zip(outs[0], outs[1], ("action_seq", "state_seq", "_costs", "particle_costs")):
                if want is not None:
                    assert torch.equal(got, want), (name, tick, what)
            x0 = outs[0][1][0, 1].clone()


# ------------------------------------------------------------------------------ 3. the nominal rule
def test_everything_outside_the_particle_rollout_is_the_nominal_members():
    cs = EC.case("mlp41_relu_2l_res")
    T, N, members = 8, 65, [2, 0, 0, 2, 0]  # (never member 1)
    a, b = ERig(cs, T, N, nominal=1), ERig(cs, T, N, member=1)
    mean = a_mean(cs, T, 5)
    for nominal, idx in ((1, 3), (2, 4)):
        if nominal == 2:
            a.ens.set_nominal(2)
            a.solver._refresh_model_inputs()          # what every forward() does first: mppi_set_mlp_nominal
            b.put_table(cs["tables"][2])
        n, nom = C.c_int(-1), C.c_int(-1)
        a.h.call("mppi_get_mlp_ensemble", C.byref(n), C.byref(nom))
        assert (n.value, nom.value) == (3, nominal)
        a.set_mean(mean), b.set_mean(mean)
        put_particles(a.h, EC.PARTS)
        a.members(members)
        act, states, stats, c = a.solve(idx, LAM)
        assert took(a.h) == (0, 0)
        M = matrix_of(a.h, EC.P, N)
        same_bits("folded", c, _host.fold_particle_costs(M, "mean"))
        same_bits(f"nominal {nominal}: state_seq", states, b.states_of(act))
        same_bits(f"nominal {nominal}: mppi_rollout_actions", a.states_of(act), b.states_of(act))
        other = ERig(cs, T, N, member=0)
        assert not np.array_equal(states, other.states_of(act)), "another member's state sequence differs"
        other.close()
        # get_top_samples: the plain handle, given the folded costs of the same solve
        b.rollout(idx)                                 # (its snapshots: the nominal state and the mean)
        b.h.call("mppi_set_costs", np.ascontiguousarray(c).ctypes.data_as(C.c_void_p), 0, stream())
        same_bits(f"nominal {nominal}: top states", a.top_states(8, LAM), b.top_states(8, LAM))
    a.close(), b.close()


def test_a_pending_state_sequence_belongs_to_the_old_nominal_member_and_the_old_weights():
    cs = EC.case("mlp41_relu_2l_res")
    T, N = 8, 65
    x0 = torch.from_numpy(R.X0.copy()).cuda()
    b = ERig(cs, T, N, member=1)
    for change in ("set_nominal", "update_weights"):
        solver, ens = ens_solver(cs, T, N, nominal=1, lazy_state_seq=True)
        solver.set_option("math", 0), solver.set_option("fused_solve", 0)
        solver.set_state_particles(torch.from_numpy(EC.PARTS).cuda(), members=[2, 0, 0, 2, 0])
        act, states = solver.forward(x0)
        serial, pending = C.c_uint32(0), C.c_int(0)
        solver._h.call("mppi_state_seq_serial", C.byref(serial), C.byref(pending))
        assert pending.value == 1, "the multi-kernel solve left its state sequence pending"
        if change == "set_nominal":
            ens.set_nominal(2)
        else:
            ens.update_weights(1, *EC.net(4242, 1, 2))
        solver._refresh_model_inputs()                 # settles the pending sequence FIRST
        solver._h.call("mppi_state_seq_serial", C.byref(serial), C.byref(pending))
        assert pending.value == 0
        torch.cuda.synchronize()
        same_bits(f"{change}: the pending state_seq", (states + 0).cpu().numpy()[0], b.states_of(act.cpu().numpy()))
    b.close()


# ------------------------------------------------------------------------------ 4. re-upload of one member
def test_update_weights_changes_only_the_rows_of_that_member():
    cs = EC.case("mlp42_relu_2l_abs")
    T, N, members = 7, 300, list(EC.MEMBERS)
    a, b = ERig(cs, T, N), ERig(cs, T, N, member=0)
    mean = a_mean(cs, T, 9)
    a.set_mean(mean), b.set_mean(mean)
    M0, _ = particle_rows(a, EC.PARTS, members, 3)
    Ws, bs = EC.net(777, cs["dc"], cs["hidden_layers"])
    a.ens.update_weights(1, Ws, bs)
    a.solver._refresh_model_inputs()
    assert a.h.mlp_members[1] == (0, 1, 0)
    M1, _ = particle_rows(a, EC.PARTS, members, 3)
    tables = cs["tables"].copy()
    tables[1] = R.pack(Ws, bs, cs["dc"])
    want = plain_rows(b, tables, members, EC.PARTS, 3)
    for m, e in enumerate(members):
        same_bits(f"particle {m} (member {e}) after the update", M1[m], want[m])
        assert np.array_equal(M1[m], M0[m]) == (e != 1), (m, e)
    a.close(), b.close()


# ------------------------------------------------------------------------------ 5. sixteen members, sixteen particles
@pytest.mark.parametrize("name", ["mlp41_tanh_1l_res", "mlp42_relu_2l_abs"])
def test_sixteen_members_sixteen_particles(name):
    cs = EC.case(name, 16)
    T, N = 8, 65
    a, b = ERig(cs, T, N), ERig(cs, T, N, member=0)
    mean = a_mean(cs, T, 16)
    a.set_mean(mean), b.set_mean(mean)
    rng = np.random.default_rng(16)
    parts = (R.X0 + rng.normal(0.0, 0.1, (16, 4))).astype(f32)
    M = check_rows(f"{name} E=P=16", a, b, cs["tables"], list(range(16)), parts, 3, mean, 0, ("cvar", 4))
    assert len({M[m].tobytes() for m in range(16)}) == 16
    a.close(), b.close()


# ------------------------------------------------------------------------------ 6. solver level
@pytest.mark.parametrize("risk_kw", [dict(risk="mean"), dict(risk="worst"), dict(risk="cvar", risk_alpha=0.5)], ids=["mean", "worst", "cvar"])
def test_set_model_particles_is_the_state_repeated_with_the_identity_map(risk_kw):
    cs = EC.case("mlp41_tanh_1l_res")
    T, N = 8, 300
    mode, _ = ens_solver(cs, T, N, **risk_kw)
    table, _ = ens_solver(cs, T, N, **risk_kw)
    mode.set_model_particles("all")
    assert mode.model_particles == (0, 1, 2) and mode.particle_members == (0, 1, 2)
    x = torch.from_numpy(R.X0.copy()).cuda()
    for tick in range(3):
        table.set_state_particles(x.repeat(EC.E, 1), members=range(EC.E))
        a, s = mode.forward(x)
        b, r = table.forward(x)
        assert torch.equal(a, b) and torch.equal(s, r) and torch.equal(mode._costs, table._costs), tick
        assert torch.equal(mode.particle_costs, table.particle_costs), tick
        Mh = mode.particle_costs.cpu().numpy()
        k = _host.risk_k(risk_kw.get("risk_alpha", 1.0), EC.E)
        same_bits("folded", mode._costs.cpu().numpy(), _host.fold_particle_costs(Mh, risk_kw["risk"], k))
        assert not np.array_equal(Mh[0], Mh[1]) and not np.array_equal(Mh[0], Mh[2])
        assert torch.equal(mode.state_particles, x.repeat(EC.E, 1))
        x = s[0, 1].clone()
    mode.reset()                                       # a setting: it stays; an explicit table is dropped as before
    table.reset()
    assert mode.model_particles == (0, 1, 2) and mode.particle_members == (0, 1, 2) and table.particle_members is None
    mode.forward(x)
    assert mode.particle_costs.shape == (3, N)
    mode.set_state_particles(torch.from_numpy(EC.PARTS).cuda(), members=list(EC.MEMBERS))  # the later call wins
    assert mode.model_particles is None and mode.particle_members == EC.MEMBERS
    mode.set_model_particles([2, 1])
    assert mode.particle_members == (2, 1)
    mode.forward(x)
    assert mode.particle_costs.shape == (2, N)
    mode.set_model_particles(None)
    assert mode.particle_members is None and mode.state_particles is None
    mode.forward(x)
    with pytest.raises(Exception):
        mode.particle_costs


def test_essps_runs_on_the_folded_costs():
    cs = EC.case("mlp42_tanh_1l_abs")
    T, N = 7, 300
    solver, _ = ens_solver(cs, T, N, lam="ESSPS", essps_target_ess=40.0, lambda_min=0.01, lambda_max=100.0, risk="worst")
    solver.set_model_particles("all")
    solver.forward(torch.from_numpy(R.X0.copy()).cuda())
    lam = float(solver._last_lambda)
    c = solver._costs.cpu().numpy()
    same_bits("folded", c, _host.fold_particle_costs(solver.particle_costs.cpu().numpy(), "worst"))
    plain = ERig(cs, T, N, member=0)
    st = stream()
    plain.h.call("mppi_set_costs", np.ascontiguousarray(c).ctypes.data_as(C.c_void_p), 0, st)
    plain.h.call("mppi_essps_lambda_device", 40.0, 0.01, 100.0, st)
    nxt, used = C.c_double(0.0), C.c_double(0.0)
    plain.h.call("mppi_get_lambda", C.byref(nxt), C.byref(used), st)
    assert 0.01 < lam < 100.0 and lam == nxt.value, (lam, nxt.value)
    plain.close()


def test_action_cost_is_added_once_behind_the_fold():
    cs = EC.case("mlp42_relu_2l_abs")
    T, N = 8, 300
    rig = ERig(cs, T, N, action_cost=True)
    mean = a_mean(cs, T, 3)
    rig.set_mean(mean)
    put_particles(rig.h, EC.PARTS)
    rig.members(list(EC.MEMBERS))
    risk(rig.h, "cvar", 2)
    term(rig, 1.0, 3.0)
    c1 = rig.rollout(3)
    fold = _host.fold_particle_costs(matrix_of(rig.h, EC.P, N), "cvar", 2)
    U = rig.actions_around(mean)
    g = acref.g32(mean, f32(cs["sigmas"]))
    acref.check("fold + kappa * A", c1, fold, acref.kappa32(1.0, 3.0), g, U)
    assert np.any(c1 != fold)
    same_bits("minimum", [min_of(rig.h)], [c1.min()])
    rig.close()


@pytest.mark.parametrize("kw", [dict(adapt_covariance=True), dict(noise_beta=0.5)], ids=["adapt_covariance", "noise_beta"])
def test_tiles_only_noise_sources(kw):
    cs = EC.case("mlp41_relu_2l_res")
    T, N, members = 8, 300, list(EC.MEMBERS)
    a, b = ERig(cs, T, N, **kw), ERig(cs, T, N, member=0, **kw)
    mean = a_mean(cs, T, 12)
    a.set_mean(mean), b.set_mean(mean)
    risk(a.h, "cvar", 2)
    M, c = particle_rows(a, EC.PARTS, members, 3)
    want = plain_rows(b, cs["tables"], members, EC.PARTS, 3)
    for m in range(EC.P):
        same_bits(f"particle {m}", M[m], want[m])
    same_bits("folded", c, _host.fold_particle_costs(M, "cvar", 2))
    a.close(), b.close()


def test_deepcopy_and_state_dict_continue_identically():
    cs = EC.case("mlp41_tanh_1l_res")
    T, N = 8, 300
    x0 = torch.from_numpy(R.X0.copy()).cuda()
    for how in ("mode", "table"):
        solver, ens = ens_solver(cs, T, N, nominal=1, risk="cvar", risk_alpha=0.5)
        parts = torch.from_numpy(EC.PARTS).cuda()
        if how == "mode":
            solver.set_model_particles([2, 0, 1])
        else:
            solver.set_state_particles(parts, members=list(EC.MEMBERS))
        solver.forward(x0)
        twin = copy.deepcopy(solver)
        assert twin._cost_owner is not ens and twin._cost_owner.nominal == 1
        assert twin.particle_members == solver.particle_members and twin.model_particles == solver.model_particles
        third, _ = ens_solver(cs, T, N, nominal=1)
        third.load_state_dict(solver.state_dict())
        assert third.particle_members == solver.particle_members and third.model_particles == solver.model_particles
        assert third.risk == ("cvar", 0.5)
        outs = []
        for s in (solver, twin, third):
            a, st = s.forward(x0)
            outs.append((a.cpu().numpy(), st.cpu().numpy(), s._costs.cpu().numpy(), s.particle_costs.cpu().numpy()))
        for what, (g0, g1, g2) in zip(("action_seq", "state_seq", "_costs", "particle_costs"), zip(*outs)):
            same_bits(f"{how} deepcopy: {what}", g1, g0)
            same_bits(f"{how} state_dict: {what}", g2, g0)


def test_two_windows_reproduce_the_unsharded_columns():
    cs = EC.case("mlp42_tanh_1l_abs")
    T, N, members = 7, 256, list(EC.MEMBERS)
    full = ERig(cs, T, N)
    mean = a_mean(cs, T, 4)
    full.set_mean(mean)
    M, _ = particle_rows(full, EC.PARTS, members, 3)
    for off in (0, N // 2):
        half = ERig(cs, T, N // 2)
        half.window(off)
        half.set_mean(mean)
        Mh, ch = particle_rows(half, EC.PARTS, members, 3)
        same_bits(f"offset {off}", Mh, M[:, off:off + N // 2])
        same_bits(f"offset {off}: folded", ch, _host.fold_particle_costs(Mh, "mean"))
        half.close()
    full.close()


# ------------------------------------------------------------------------------ 7. errors
def test_errors():
    from mppi_playground_amd._capi import MppiError
    from test_gpu_covariance import make

    cs = EC.case("mlp41_relu_2l_res")
    T, N = 8, 65
    INVALID = r"\(-1\)"
    ints = lambda v: (C.c_int * len(v))(*v)  # noqa: E731
    # a map on a handle of another model
    nav, _ = make("nav2d", 8, 64, 1.0)
    with pytest.raises(MppiError, match=INVALID):
        nav._h.call("mppi_set_particle_members", ints([0, 0]), 2)
    nav._h.call("mppi_set_particle_members", None, 0)  # (none: nothing to refuse)
    tabs = np.ascontiguousarray(cs["tables"], f32)
    with pytest.raises(MppiError, match=INVALID):
        nav._h.call("mppi_set_mlp_ensemble", tabs.ctypes.data_as(C.c_void_p), 3, tabs.shape[1], 2, 0, 1, 0, None)
    a = ERig(cs, T, N)
    put = lambda t, E, n=tabs.shape[1], hl=2, act=0, res=1, nominal=0: a.h.call(  # noqa: E731
        "mppi_set_mlp_ensemble", t.ctypes.data_as(C.c_void_p), E, n, hl, act, res, nominal, stream())
    big = np.ascontiguousarray(np.tile(tabs[:1], (17, 1)))
    for E in (0, 17, -1):
        with pytest.raises(MppiError, match=INVALID):
            put(big, E)
    for kw in (dict(n=tabs.shape[1] - 1), dict(hl=3), dict(act=2), dict(res=2), dict(nominal=3), dict(nominal=-1)):
        with pytest.raises(MppiError, match=INVALID):
            put(tabs, 3, **kw)
    for bad in (np.nan, np.inf):
        t = tabs.copy()
        t[2, 700] = bad                                # (in the LAST member: every table is checked)
        with pytest.raises(MppiError, match=r"\(-1\).*finite"):
            put(t, 3)
        with pytest.raises(MppiError, match=r"\(-1\).*finite"):
            a.h.call("mppi_set_mlp_member", 1, t[2].ctypes.data_as(C.c_void_p), t.shape[1], stream())
    for e in (-1, 3):
        with pytest.raises(MppiError, match=INVALID):
            a.h.call("mppi_set_mlp_member", e, tabs[0].ctypes.data_as(C.c_void_p), tabs.shape[1], stream())
        with pytest.raises(MppiError, match=INVALID):
            a.h.call("mppi_set_mlp_nominal", e)
    # a length mismatch is found at the rollout, with either call order; so is an entry >= E
    a.h.call("mppi_sample", 3, stream())
    put_particles(a.h, EC.PARTS)
    a.members([0, 1, 2])
    with pytest.raises(MppiError, match=r"\(-1\).*particle members"):
        a.h.call("mppi_rollout_cost", stream())
    a.h.call("mppi_set_particles", None, 0, 0, stream())    # (off: the map goes with it)
    n = C.c_int(-1)
    a.h.call("mppi_get_particle_members", None, C.byref(n))
    assert n.value == 0
    a.members([0, 1, 2])
    put_particles(a.h, EC.PARTS)
    with pytest.raises(MppiError, match=r"\(-1\).*particle members"):
        a.h.call("mppi_rollout_cost", stream())
    a.members([0, 1, 3, 0, 0])
    with pytest.raises(MppiError, match=r"\(-1\).*particle members"):
        a.h.call("mppi_rollout_cost", stream())
    with pytest.raises(MppiError, match=INVALID):
        a.members([0, -1, 0, 0, 0])
    with pytest.raises(MppiError, match=INVALID):
        a.members([0] * 17)
    a.members(list(EC.MEMBERS))
    a.h.call("mppi_rollout_cost", stream())            # now it runs
    torch.cuda.synchronize()
    assert np.all(np.isfinite(matrix_of(a.h, EC.P, N)))
    # the solver
    solver = a.solver
    parts = torch.from_numpy(EC.PARTS)
    for bad in ([0, 1, 2], [0, 1, 2, 3, 0], [0, 1, 2, -1, 0], "some"):
        with pytest.raises(ValueError, match="members"):
            solver.set_state_particles(parts, members=bad)
    for bad in ([3], [0] * 17, [], "some"):
        with pytest.raises(ValueError, match="members"):
            solver.set_model_particles(bad)
    plain, _ = member_solver(cs, 0, T, N)              # a model that is no ensemble
    with pytest.raises(ValueError, match="MLPEnsemble"):
        plain.set_state_particles(parts, members=list(EC.MEMBERS))
    with pytest.raises(ValueError, match="MLPEnsemble"):
        plain.set_model_particles("all")
    with pytest.raises(ValueError, match="MLPEnsemble"):
        nav.set_model_particles("all")
    from pi_mpc.mppi import MPPI

    ens = a.ens
    opaque = MPPI(dynamics=lambda s, u: ens.dynamics(s, u), cost_func=lambda s, u, i: ens.cost(s, u, i), **common(cs, T, N, LAM))
    assert opaque._model is None
    with pytest.raises(ValueError, match="opaque"):
        opaque.set_state_particles(parts, members=list(EC.MEMBERS))
    with pytest.raises(ValueError, match="opaque"):
        opaque.set_model_particles("all")
    # mismatched architectures never reach the device
    from envs import MLPEnsemble

    with pytest.raises(ValueError):
        MLPEnsemble(EC.models(cs)[:1] + EC.models(EC.case("mlp41_tanh_1l_res"))[:1])
    a.close()
