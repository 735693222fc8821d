"""Risk-aware solves (mppi_set_particles: every sample rolled out from a set of start states, its P costs folded by a risk
measure) on a real MI355X.

The solver is its own oracle: the noise of a sample does not depend on the start state, so row m of the [P, N] matrix must
equal, BIT FOR BIT at math level 0, what a plain handle of the same model, seed and solve index computes from
x0 = particles[m] around the same mean.  At the fast levels (item 3) no new tolerance is introduced: every row is held to the
yardstick and limit the model's existing test applies to rollout_cost_kernel — the oracle and test_gpu_parity.check_costs for
nav2d and racing, the float64 restatement and test_gpu_moving_discs.in_parity for the disc model — particle by particle; how
many values equal the plain kernel's bits is printed, not asserted.  The fold is held to pi_mpc._host.fold_particle_costs bit
for bit on injected matrices (tests/particle_cases.py) and the minimum the solve then uses to min() of the folded vector.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import action_cost_ref as acref
import particle_cases as pc
from helpers import MODEL_CFG, oracle_problem
from pi_mpc import _host
from test_gpu_action_cost import LAM, Rig, random_mean, sigmas_of, term
from test_gpu_covariance import _need_gpu, make, weights64
from test_gpu_fused_geometry import took

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
MEAN, WORST, CVAR = 0, 1, 2
MODE_ID = {"mean": MEAN, "worst": WORST, "cvar": CVAR}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(name, got, want):
    bad = int(np.sum(bits(got) != bits(want)))
    assert bad == 0, f"{name}: {bad} of {np.size(got)} values differ"


def stream():
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(0))


# ------------------------------------------------------------------------------ handles through the C ABI
def put_particles(h, parts, on_device=False):
    parts = np.ascontiguousarray(parts, f32)
    if on_device:
        h._parts_keep = torch.from_numpy(parts).cuda()
        h.call("mppi_set_particles", h._parts_keep.data_ptr(), parts.shape[0], 1, stream())
    else:
        h.call("mppi_set_particles", parts.ctypes.data_as(C.c_void_p), parts.shape[0], 0, stream())


def risk(h, mode, k=1):
    h.call("mppi_set_risk", MODE_ID.get(mode, mode), int(k))


def matrix_of(h, P, N):
    m = torch.empty(P, N, device="cuda")
    h.call("mppi_get_particle_costs", m.data_ptr(), 1, stream())
    return m.cpu().numpy()


def costs_of(h, N):
    c = torch.empty(N, device="cuda")
    h.call("mppi_get_costs", c.data_ptr(), 1, stream())
    return c.cpu().numpy()


def min_of(h):
    """The minimum the solve uses: {min c, ...} of mppi_softmax_stats, as the fp32 it is"""
    out = (C.c_double * 5)()
    h.call("mppi_softmax_stats", 1.0, out, stream())
    return f32(out[0])


def set_state(rig, x):
    rig._x_keep = torch.from_numpy(np.ascontiguousarray(x, f32)).cuda()
    rig.h.call("mppi_set_state", rig._x_keep.data_ptr(), 1, stream())


def plain_rows(plain, parts, idx):
    """[P, N]: the plain handle's costs of solve `idx` from every particle as ITS start state"""
    rows = []
    for x in parts:
        set_state(plain, x)
        rows.append(plain.rollout(idx))
    return np.stack(rows)


def particle_rows(rig, parts, idx, on_device=False):
    """([P, N] matrix, folded costs [N]) of solve `idx` with `parts` set; the nominal state stays the rig's own"""
    put_particles(rig.h, parts, on_device)
    c = rig.rollout(idx)
    return matrix_of(rig.h, len(parts), rig.N), c


def pair(model, T, N, math=0, **kw):
    a, b = Rig(model, T, N, **kw), Rig(model, T, N, **kw)
    for r in (a, b):
        r.h.call("mppi_set_option", b"math", math)
        r.h.call("mppi_set_option", b"fused_solve", 0)
    return a, b


def both_means(a, b, seed, scale=0.3):
    mean = (random_mean(a, seed) * scale).astype(f32)
    a.set_mean(mean)
    b.set_mean(mean)
    return mean


def generic_handle(N, T=3, ds=5, dc=2):
    _need_gpu()
    from mppi_playground_amd import _capi

    cfg = _capi.MppiConfig()
    cfg.model, cfg.horizon, cfg.dim_state, cfg.dim_control = _capi.MODEL_GENERIC, T, ds, dc
    cfg.num_samples, cfg.sample_offset, cfg.inherit_count = N, 0, N
    for k in range(dc):
        cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = -1.0, 1.0, 0.5
    cfg.seed, cfg.device = 42, 0
    return _capi.Handle(cfg)


# ------------------------------------------------------------------------------ 1. the fold on injected matrices
@pytest.mark.parametrize("N", pc.SIZES_N)
@pytest.mark.parametrize("kind", ["generic", "nav2d"])
def test_fold_on_injected_matrices(kind, N):
    if kind == "generic":
        h, keep = generic_handle(N), None
    else:
        keep = Rig("nav2d", 2, N)
        h = keep.h
    checked = 0
    for P in pc.SIZES_P:
        put_particles(h, np.zeros((P, 5 if kind == "generic" else 3), f32), on_device=bool(P & 1))
        for shape in pc.KINDS:
            m = pc.matrix(shape, P, N)
            dev = torch.from_numpy(m).cuda()
            for mode in pc.MODES:
                for k in (pc.ks(P) if mode == "cvar" else (1,)):
                    risk(h, mode, k)
                    if checked & 1:  # (host and device sources alternate)
                        h.call("mppi_set_particle_costs", m.ctypes.data_as(C.c_void_p), 0, stream())
                    else:
                        h.call("mppi_set_particle_costs", dev.data_ptr(), 1, stream())
                    want = _host.fold_particle_costs(m, mode, k)
                    name = f"{kind} N={N} P={P} {shape} {mode} k={k}"
                    same_bits(name, costs_of(h, N), want)
                    same_bits(name + ": minimum", [min_of(h)], [want.min()])
                    same_bits(name + ": matrix read back", matrix_of(h, P, N), m)
                    checked += 1
    assert checked == len(pc.KINDS) * sum(2 + len(pc.ks(P)) for P in pc.SIZES_P)
    h.close()


@pytest.mark.parametrize("N", [65, 300])
def test_two_folds_in_a_row_keep_the_minimum_key(N):
    """The double-buffered key: a smaller minimum first, then a larger one, then a smaller one again (no memset in between)."""
    h = generic_handle(N)
    P = 3
    put_particles(h, np.zeros((P, 5), f32))
    risk(h, "worst")
    base = pc.matrix("mixed", P, N)
    for shift in (-1000.0, 500.0, 2000.0, -3.0):
        m = (base + f32(shift)).astype(f32)
        h.call("mppi_set_particle_costs", m.ctypes.data_as(C.c_void_p), 0, stream())
        want = _host.fold_particle_costs(m, "worst")
        same_bits(f"shift {shift}", costs_of(h, N), want)
        same_bits(f"shift {shift}: minimum", [min_of(h)], [want.min()])
    # ... and next to the vector's own setter
    v = pc.matrix("mixed", 1, N)[0] + f32(7.0)
    h.call("mppi_set_costs", v.ctypes.data_as(C.c_void_p), 0, stream())
    same_bits("set_costs: minimum", [min_of(h)], [v.min()])
    h.call("mppi_set_particle_costs", base.ctypes.data_as(C.c_void_p), 0, stream())
    same_bits("after set_costs: minimum", [min_of(h)], [_host.fold_particle_costs(base, "worst").min()])
    h.close()


# ------------------------------------------------------------------------------ 2. per-particle costs against the plain solver, math 0
NAV_PARTS = f32([[-9.0, -9.0, 0.785], [-40.0, -9.0, 0.785], [-8.6, -9.3, 0.6]])  # the second lies outside the position clamp


def racing_parts(rig, P=3):
    x = rig.x0.cpu().numpy()
    d = f32([[0.0, 0.0, 0.0, 0.0], [0.4, -0.3, 0.05, 0.5], [-0.5, 0.2, -0.08, -0.3], [0.1, 0.1, 0.0, 0.0]])
    return (x[None, :] + d[:P]).astype(f32)


def check_rows_both_noise_paths(name, a, b, parts, idx, fold=("mean", 1)):
    """Row m of the particle handle == the plain handle from particles[m], with regenerated noise and with tiles; the folded
    vector == the restatement of the matrix; the matrices of the two noise paths agree."""
    mats = []
    for regen in (1, 0):
        for r in (a, b):
            r.h.call("mppi_set_option", b"noise_regen", regen)
        risk(a.h, *fold)
        M, c = particle_rows(a, parts, idx, on_device=bool(regen))
        want = plain_rows(b, parts, idx)
        assert np.all(np.isfinite(M)), name
        for m in range(len(parts)):
            same_bits(f"{name} regen={regen} particle {m}", M[m], want[m])
        same_bits(f"{name} regen={regen}: folded", c, _host.fold_particle_costs(M, *fold))
        same_bits(f"{name} regen={regen}: minimum", [min_of(a.h)], [c.min()])
        mats.append(M)
    same_bits(f"{name}: regenerated noise against tiles", mats[0], mats[1])
    return mats[0]


@pytest.mark.parametrize("T", [7, 8])
def test_nav2d_rows_with_one_particle_outside_the_clamp(T):
    a, b = pair("nav2d", T, 300)
    both_means(a, b, T)
    M = check_rows_both_noise_paths(f"nav2d T={T}", a, b, NAV_PARTS, 3, ("cvar", 2))
    assert not np.array_equal(M[0], M[1]) and not np.array_equal(M[0], M[2])
    a.close(), b.close()


@pytest.mark.parametrize("T", [15, 16])
def test_pendulum_rows(T):
    a, b = pair("pendulum", T, 200)
    both_means(a, b, T)
    check_rows_both_noise_paths(f"pendulum T={T}", a, b, f32([[3.0, 0.1], [-2.0, 1.5]]), 4, ("worst", 1))
    a.close(), b.close()


def test_racing_rows_with_exploration():
    a, b = pair("racing", 8, 256, exploration=0.3)
    both_means(a, b, 5)
    M = check_rows_both_noise_paths("racing", a, b, racing_parts(a), 5, ("mean", 1))
    assert not np.array_equal(M[0], M[1])
    a.close(), b.close()


def disc_pair(T, N, math):
    import discs_ref as D
    from test_gpu_moving_discs import DiscRig

    table = D._crossing(T, 2)
    rigs = [DiscRig(table, D.X0, T, N, math=math) for _ in range(2)]
    for r in rigs:
        r.h.call("mppi_set_option", b"fused_solve", 0)
    parts = f32([D.X0, D.X0 + f32([0.05, -0.04, 0.03])])
    return rigs[0], rigs[1], parts


def test_disc_model_rows():
    a, b, parts = disc_pair(8, 128, 0)
    check_rows_both_noise_paths("nav2d_discs", a, b, parts, 3, ("cvar", 1))
    a.close(), b.close()


def test_mlp_rows():
    import mlp_ref
    from test_gpu_mlp_model import MlpRig

    cs = mlp_ref.case("mlp41_relu_2l_res")
    a, b = MlpRig(cs, 5, 64), MlpRig(cs, 5, 64)
    b.set_mean(a.mean0)
    for r in (a, b):
        r.h.call("mppi_set_option", b"fused_solve", 0)
    parts = f32([mlp_ref.X0, mlp_ref.X0 + f32([0.1, -0.05, 0.02, 0.03])])
    check_rows_both_noise_paths("mlp41", a, b, parts, 3, ("mean", 1))
    a.close(), b.close()


def test_sixteen_particles():
    a, b = pair("nav2d", 8, 64)
    both_means(a, b, 16)
    rng = np.random.default_rng(16)
    parts = (NAV_PARTS[0] + rng.normal(0.0, 0.3, (16, 3))).astype(f32)
    parts[7] = NAV_PARTS[1]
    check_rows_both_noise_paths("nav2d P=16", a, b, parts, 3, ("cvar", 4))
    a.close(), b.close()


# ------------------------------------------------------------------------------ 3. the fast math levels
def count_equal(name, M, want):
    eq = int(np.sum(bits(M) == bits(want)))
    print(f"[particles] {name}: {eq} of {M.size} values equal the plain kernel's bit for bit")


@pytest.mark.parametrize("math", [1, 2])
@pytest.mark.parametrize("model,T,N", [("nav2d", 8, 300), ("racing", 8, 256)])
def test_fast_levels_against_the_oracle(model, T, N, math):
    """Row m against the oracle's rollout from particles[m] on the exported noise: test_gpu_parity.check_costs, as it stands."""
    from test_gpu_parity import check_costs

    a, b = pair(model, T, N, math=math)
    mean = both_means(a, b, 11)
    parts = NAV_PARTS if model == "nav2d" else racing_parts(a)
    M, _ = particle_rows(a, parts, 6)
    count_equal(f"{model} math {math}", M, plain_rows(b, parts, 6))
    eps = torch.empty(N, T, a.dc, device="cuda")
    a.h.call("mppi_export_noise", eps.data_ptr(), None, stream())
    eps = eps.cpu().numpy()
    P = oracle_problem(model, N, T)
    if model == "racing":
        ref = a.solver._ref_uploaded
        P.set_ref_path(np.ascontiguousarray(ref.cpu().numpy() if torch.is_tensor(ref) else ref, f32))
    for m, x in enumerate(parts):
        check_costs(M[m], P.rollout_cost(x, mean, eps, want_margin=True))
    a.close(), b.close()


def test_pendulum_particle_whose_lanes_redo_at_the_default_level():
    """One particle far outside the fast path's range (a start of the existing extreme-state cases: lanes redo with the
    library math), at the DEFAULT math level: held to that test's yardstick and limit (the oracle, 1e-4 of the scale)."""
    T, N = 15, 200
    a, b = Rig("pendulum", T, N), Rig("pendulum", T, N)
    mean = both_means(a, b, 2)
    parts = f32([[3.0, 0.1], [150.0, -3.0]])
    M, _ = particle_rows(a, parts, 4)
    count_equal("pendulum redo", M, plain_rows(b, parts, 4))
    eps = torch.empty(N, T, 1, device="cuda")
    a.h.call("mppi_export_noise", eps.data_ptr(), None, stream())
    eps = eps.cpu().numpy()
    P = oracle_problem("pendulum", N, T)
    for m, x in enumerate(parts):
        r = P.rollout_cost(x, mean, eps, want_margin=True)
        scale = max(np.abs(r["costs"]).max(), 1e-30)
        assert np.all(np.isfinite(M[m]))
        assert np.abs(M[m] - r["costs"]).max() <= 1e-4 * scale, (m, np.abs(M[m] - r["costs"]).max() / scale)
    a.close(), b.close()


@pytest.mark.parametrize("math", [1, 2])
def test_disc_model_fast_levels_within_the_parity_rule(math):
    from test_gpu_moving_discs import in_parity

    a, b, parts = disc_pair(8, 128, math)
    M, _ = particle_rows(a, parts, 3)
    count_equal(f"nav2d_discs math {math}", M, plain_rows(b, parts, 3))
    U = a.actions_around(a.mean0)
    for m, x in enumerate(parts):
        a.x0_host = f32(x)  # (DiscRig.ref rolls out from it)
        in_parity(f"particle {m} math {math}", a, M[m], U)
    a.close(), b.close()


# ------------------------------------------------------------------------------ 4. end to end
def finalize_from_costs(rig, idx, costs, lam):
    """A plain handle given `costs` for solve `idx`: mppi_set_costs, mppi_weights_reduce, mppi_finalize -> (action, states, stats)"""
    st = stream()
    rig.h.call("mppi_sample", idx, st)
    c = np.ascontiguousarray(costs, f32)
    rig.h.call("mppi_set_costs", c.ctypes.data_as(C.c_void_p), 0, st)
    rig.h.call("mppi_weights_reduce", float(lam), None, st)
    rig.h.call("mppi_finalize", None, 1, float(lam), 1, rig.action.data_ptr(), rig.state.data_ptr(), rig.stats.data_ptr(), st)
    torch.cuda.synchronize()
    return rig.action.cpu().numpy(), rig.state.cpu().numpy()[0], rig.stats.cpu().numpy()


@pytest.mark.parametrize("mode,k", [("mean", 1), ("worst", 1), ("cvar", 2)])
def test_solve_equals_a_plain_handle_given_the_folded_costs(mode, k):
    T, N, lam = 8, 300, 5.0
    a, b = Rig("nav2d", T, N), Rig("nav2d", T, N, )
    b.h.call("mppi_set_option", b"fused_solve", 0)
    both_means(a, b, 8)
    put_particles(a.h, NAV_PARTS)
    risk(a.h, mode, k)
    act, states, stats, c = a.solve(3, lam)
    assert took(a.h) == (0, 0), "particles take the multi-kernel sequence"
    same_bits("folded", c, _host.fold_particle_costs(matrix_of(a.h, 3, N), mode, k))
    act_b, states_b, stats_b = finalize_from_costs(b, 3, c, lam)
    same_bits("action_seq", act, act_b)      # (both took the multi-kernel sequence)
    same_bits("state_seq", states, states_b)
    same_bits("stats", stats, stats_b)
    same_bits("minimum", [stats[0]], [c.min()])
    same_bits("state_seq[0] is the nominal state", states[0], a.x0.cpu().numpy())
    e, ess = weights64(c, lam)
    assert ess > 3.0
    a.close(), b.close()


def test_switching_off_is_the_solver_that_never_had_particles():
    T, N, lam = 8, 300, 5.0
    a, b = Rig("nav2d", T, N), Rig("nav2d", T, N)
    both_means(a, b, 9)
    put_particles(a.h, NAV_PARTS)
    a.solve(2, lam)
    assert took(a.h) == (0, 0)
    a.set_mean(b.mean())                                        # (the solve stored its plan: back to the common warm start)
    a.h.call("mppi_set_particles", None, 0, 0, stream())
    act, states, stats, c = a.solve(3, lam)
    act_b, states_b, stats_b, c_b = b.solve(3, lam)
    assert took(a.h) == took(b.h) and took(b.h) != (0, 0), "back to the single launch"
    same_bits("costs", c, c_b)
    same_bits("action_seq", act, act_b)
    same_bits("state_seq", states, states_b)
    a.close(), b.close()


@pytest.mark.parametrize("model,T,N", [("nav2d", 8, 300), ("racing", 8, 256)])
def test_one_particle_at_the_state_is_the_plain_solve(model, T, N):
    lam = 5.0
    a, b = pair(model, T, N, math=2)
    for idx, (mode, k) in enumerate([("mean", 1), ("worst", 1), ("cvar", 1)]):
        both_means(a, b, 20 + idx)
        put_particles(a.h, a.x0.cpu().numpy()[None, :], on_device=True)
        risk(a.h, mode, k)
        act, states, stats, c = a.solve(3 + idx, lam)
        act_b, states_b, stats_b, c_b = b.solve(3 + idx, lam)
        assert took(a.h) == (0, 0) and took(b.h) == (0, 0)
        same_bits(f"{mode}: costs", c, c_b)
        same_bits(f"{mode}: action_seq", act, act_b)
        same_bits(f"{mode}: state_seq", states, states_b)
        same_bits(f"{mode}: stats", stats, stats_b)
    a.close(), b.close()


# ------------------------------------------------------------------------------ 5. around it
def nav_solver(N=300, T=8, lam=5.0, **kw):
    solver, x0 = make("nav2d", T, N, lam, **kw)
    return solver, x0.cuda()


def test_top_samples_are_the_smallest_folded_costs_from_the_nominal_state():
    solver, x0 = nav_solver(risk="cvar", risk_alpha=0.5)
    plain, _ = nav_solver()
    solver.set_state_particles(torch.from_numpy(NAV_PARTS))       # a host table
    assert solver._particles_P == 3
    solver.forward(x0)
    plain.forward(x0)
    M = solver.particle_costs.cpu().numpy()
    c = solver._costs.cpu().numpy()
    same_bits("folded", c, _host.fold_particle_costs(M, "cvar", 2))
    states, w = solver.get_top_samples(8)
    order = np.argsort(c, kind="stable")[:8]
    assert len(np.unique(c[order])) == 8, "the eight smallest folded costs are distinct"
    e, _ = weights64(c, 5.0)
    assert np.allclose(w.cpu().numpy(), (e / e.sum())[order], rtol=1e-5, atol=0)
    # (the first solve of both solvers: same seed, solve index and zero warm start -> the same actions; the particles decide
    # costs only, the re-roll starts from the nominal state)
    same_bits("top states", states.cpu().numpy(), plain._state_seq_batch.cpu().numpy()[order])
    same_bits("their start", states.cpu().numpy()[:, 0, :], np.broadcast_to(x0.cpu().numpy(), (8, 3)))


def test_deepcopy_and_state_dict_continue_identically():
    solver, x0 = nav_solver(risk="worst")
    parts = torch.from_numpy(NAV_PARTS).cuda()
    solver.set_state_particles(parts)
    a, _ = solver.forward(x0)
    twin = copy.deepcopy(solver)
    assert twin.risk == ("worst", 1.0) and twin._particles_P == 3
    same_bits("matrix copied", twin.particle_costs.cpu().numpy(), solver.particle_costs.cpu().numpy())
    same_bits("table copied", twin.state_particles.cpu().numpy(), NAV_PARTS)
    third, _ = nav_solver()
    third.load_state_dict(solver.state_dict())
    assert third.risk == ("worst", 1.0) and third._particles_P == 3
    outs = [s.forward(x0)[0].cpu().numpy() for s in (solver, twin, third)]
    same_bits("deepcopy", outs[1], outs[0])
    same_bits("state_dict", outs[2], outs[0])
    same_bits("matrix", twin.particle_costs.cpu().numpy(), solver.particle_costs.cpu().numpy())
    solver.reset()
    assert solver.risk == ("worst", 1.0) and solver._particles_P == 0 and solver.state_particles is None
    solver.forward(x0)
    g, s = C.c_int(-1), C.c_int(-1)
    solver._h.call("mppi_fused_geometry", C.byref(g), C.byref(s))
    assert g.value > 0, "reset() drops the particles: the single launch again"
    twin.set_risk("cvar", 0.3)  # k = ceil(0.9) = 1: the worst case
    twin.set_state_particles(parts)
    twin.forward(x0)
    same_bits("cvar(1) is worst", twin._costs.cpu().numpy(), _host.fold_particle_costs(twin.particle_costs.cpu().numpy(), "worst"))


def test_essps_runs_on_the_folded_costs():
    N, T = 300, 8
    kw = dict(essps_target_ess=40.0, lambda_min=0.01, lambda_max=100.0)
    solver, x0 = nav_solver(N, T, "ESSPS", risk="mean", **kw)
    solver.set_state_particles(torch.from_numpy(NAV_PARTS).cuda())
    solver.forward(x0)
    lam = float(solver._last_lambda)
    c = solver._costs.cpu().numpy()
    same_bits("folded", c, _host.fold_particle_costs(solver.particle_costs.cpu().numpy(), "mean"))
    plain = Rig("nav2d", T, N)
    st = stream()
    plain.h.call("mppi_set_costs", np.ascontiguousarray(c).ctypes.data_as(C.c_void_p), 0, st)
    plain.h.call("mppi_essps_lambda_device", 40.0, 0.01, 100.0, st)
    nxt, used = C.c_double(0.0), C.c_double(0.0)
    plain.h.call("mppi_get_lambda", C.byref(nxt), C.byref(used), st)
    assert 0.01 < lam < 100.0 and lam == nxt.value, (lam, nxt.value)
    plain.close()


@pytest.mark.parametrize("kw", [dict(adapt_covariance=True), dict(noise_beta=0.5)], ids=["adapt_covariance", "noise_beta"])
def test_tiles_only_noise_sources(kw):
    a, b = pair("nav2d", 8, 300, **kw)
    both_means(a, b, 12)
    for r in (a, b):
        r.h.call("mppi_set_option", b"noise_regen", 1)  # (these handles materialise the noise whatever the option says)
    put_particles(a.h, NAV_PARTS)
    risk(a.h, "cvar", 2)
    c = a.rollout(3)
    M = matrix_of(a.h, 3, 300)
    want = plain_rows(b, NAV_PARTS, 3)
    for m in range(3):
        same_bits(f"particle {m}", M[m], want[m])
    same_bits("folded", c, _host.fold_particle_costs(M, "cvar", 2))
    a.close(), b.close()


def test_action_cost_is_added_once_behind_the_fold():
    T, N = 8, 200
    rig = Rig("nav2d", T, N)
    mean = random_mean(rig, 3)
    rig.set_mean(mean)
    put_particles(rig.h, NAV_PARTS)
    risk(rig.h, "cvar", 2)
    term(rig, 1.0, LAM)
    c1 = rig.rollout(3)
    fold = _host.fold_particle_costs(matrix_of(rig.h, 3, N), "cvar", 2)
    U = rig.actions_around(mean)
    g = acref.g32(mean, sigmas_of(rig))
    acref.check("fold + kappa * A", c1, fold, acref.kappa32(1.0, LAM), g, U)
    assert np.any(c1 != fold)
    same_bits("minimum", [min_of(rig.h)], [c1.min()])
    rig.close()


def test_two_windows_reproduce_the_unsharded_columns():
    T, N = 8, 256
    full = Rig("nav2d", T, N)
    mean = (random_mean(full, 4) * 0.3).astype(f32)
    full.set_mean(mean)
    M, _ = particle_rows(full, NAV_PARTS, 3)
    for off in (0, N // 2):
        half = Rig("nav2d", T, N // 2)
        half.window(off)
        half.set_mean(mean)
        Mh, ch = particle_rows(half, NAV_PARTS, 3)
        same_bits(f"offset {off}", Mh, M[:, off:off + N // 2])
        same_bits(f"offset {off}: folded", ch, _host.fold_particle_costs(Mh, "mean"))
        half.close()
    full.close()


def test_generic_path_runs_the_callables_once_per_particle():
    """The nav2d callables behind untagged lambdas: the library folds the callables' own [P, N] matrix.  The plan is held to
    the limit of the existing generic-against-native test (test_gpu_moving_discs: each solver within 1e-5 of the float64
    softmax over its own costs and clamped actions); how far the two plans and matrices lie apart is printed."""
    _need_gpu()
    from envs.navigation_2d import Navigation2DEnv
    from pi_mpc.mppi import MPPI

    T, N, lam = 8, 128, 10.0
    env = Navigation2DEnv()
    cfg = MODEL_CFG["nav2d"]
    common = dict(horizon=T, num_samples=N, dim_state=3, dim_control=2, u_min=torch.tensor(cfg["u_min"]),
                  u_max=torch.tensor(cfg["u_max"]), sigmas=torch.tensor(cfg["sigmas"]), lambda_=lam, risk="cvar", risk_alpha=0.5)
    native = MPPI(dynamics=env.dynamics, cost_func=env.cost_function, **common)
    opaque = MPPI(dynamics=lambda s, a: env.dynamics(s, a), cost_func=lambda s, a, i: env.cost_function(s, a, i), **common)
    assert native._model == "nav2d" and opaque._model is None
    x0 = torch.tensor([-9.0, -9.0, 0.785]).cuda()
    parts = torch.from_numpy(f32([[-9.0, -9.0, 0.785], [-8.7, -9.2, 0.7], [-9.2, -8.8, 0.9]])).cuda()
    acts = []
    for s in (native, opaque):
        s.set_state_particles(parts)
        a, states = s.forward(x0)
        M, c = s.particle_costs.cpu().numpy(), s._costs.cpu().numpy()
        same_bits(f"{s._model}: folded", c, _host.fold_particle_costs(M, "cvar", 2))
        U = s._perturbed_action_seqs.cpu().numpy()
        e, ess = weights64(c, lam)
        assert ess > 5.0
        a64 = np.tensordot(e, U.astype(f64), axes=1) / e.sum()
        assert np.max(np.abs(a.cpu().numpy() - a64)) <= 1e-5, s._model
        same_bits(f"{s._model}: state_seq[0]", states.cpu().numpy()[0, 0], x0.cpu().numpy())
        acts.append(a.cpu().numpy())
    scale = max(np.abs(native.particle_costs.cpu().numpy()).max(), 1e-30)
    err = np.abs(opaque.particle_costs.cpu().numpy() - native.particle_costs.cpu().numpy()).max() / scale
    print(f"[particles] generic against native: matrices within {err:.3g} of the scale, plans within {np.abs(acts[0] - acts[1]).max():.3g}")
    ts, _ = opaque.get_top_samples(4)
    same_bits("generic top samples start at the nominal state", ts.cpu().numpy()[:, 0, :], np.broadcast_to(x0.cpu().numpy(), (4, 3)))


def test_captured_callables_are_replayed_once_per_particle():
    """graph_callables=True with particles: the captured loops read the start state from a static buffer, so the graph is
    replayed once per particle — same bits as the eager loops over a closed loop (warm-up, capture, replays)."""
    _need_gpu()
    from envs import classic_control as cc
    from pi_mpc.mppi import MPPI

    cfg = MODEL_CFG["pendulum"]
    make_one = lambda **kw: MPPI(horizon=12, num_samples=256, dim_state=2, dim_control=1,  # noqa: E731
                                 dynamics=lambda s, a: cc.pendulum_dynamics(s, a), cost_func=lambda s, a, i: cc.pendulum_cost(s, a, i),
                                 u_min=torch.tensor(cfg["u_min"]), u_max=torch.tensor(cfg["u_max"]), sigmas=torch.tensor(cfg["sigmas"]),
                                 lambda_=0.5, risk="worst", recognize_closures=False, **kw)
    eager, graph = make_one(), make_one(graph_callables=True)
    assert eager._model is None and graph._model is None
    x = torch.tensor([3.0, 0.1]).cuda()
    spread = torch.tensor([[0.0, 0.0], [0.2, -0.3], [-0.15, 0.4]]).cuda()
    for tick in range(5):
        for s in (eager, graph):
            s.set_state_particles(x + spread)
        ae, se = eager.forward(x)
        ag, sg = graph.forward(x)
        assert torch.equal(ae, ag) and torch.equal(se, sg), tick
        assert torch.equal(eager.particle_costs, graph.particle_costs) and torch.equal(eager._costs, graph._costs), tick
        same_bits(f"tick {tick}: folded", graph._costs.cpu().numpy(),
                  _host.fold_particle_costs(graph.particle_costs.cpu().numpy(), "worst"))
        x = se[0, 1].clone()
    assert graph._graph_state == "replay"
    rows = graph.particle_costs.cpu().numpy()
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[0], rows[2])


def test_errors():
    from mppi_playground_amd._capi import MppiError

    rig = Rig("nav2d", 8, 64)
    with pytest.raises(MppiError, match="mppi_set_particles"):
        put_particles(rig.h, np.zeros((17, 3), f32))
    bad = NAV_PARTS.copy()
    bad[1, 1] = np.nan
    with pytest.raises(MppiError, match="finite"):
        put_particles(rig.h, bad)
    with pytest.raises(MppiError, match="mppi_get_particle_costs"):
        matrix_of(rig.h, 3, 64)                      # none set
    with pytest.raises(MppiError, match="mppi_set_risk"):
        risk(rig.h, 3)
    put_particles(rig.h, NAV_PARTS)
    risk(rig.h, "cvar", 5)                           # either call may come first: refused where the fold is launched
    rig.h.call("mppi_sample", 3, stream())
    with pytest.raises(MppiError, match="CVAR"):
        rig.h.call("mppi_rollout_cost", stream())
    with pytest.raises(MppiError, match="CVAR"):
        rig.h.call("mppi_set_particle_costs", pc.matrix("mixed", 3, 64).ctypes.data_as(C.c_void_p), 0, stream())
    risk(rig.h, "cvar", 3)
    rig.h.call("mppi_rollout_cost", stream())
    with pytest.raises(MppiError, match="mapping"):
        rig.h.call("mppi_set_option", b"mapping", 1)
    rig.h.call("mppi_set_particles", None, 0, 0, stream())
    rig.h.call("mppi_set_option", b"mapping", 1)
    with pytest.raises(MppiError, match="mapping"):
        put_particles(rig.h, NAV_PARTS)
    solver = rig.solver
    for t in (torch.zeros(17, 3), torch.zeros(3, 4), torch.zeros(3)):
        with pytest.raises(ValueError, match="state particles"):
            solver.set_state_particles(t)
    with pytest.raises(ValueError, match="risk"):
        solver.set_risk("cvar", 1.5)
    rig.close()


# ------------------------------------------------------------------------------ 6. sanity of the measure
def test_ordering_of_the_measures():
    """One particle that starts next to an obstacle and heads for it, two that start clear.  Per sample, exactly:
    WORST >= CVAR(2) >= CVAR(3) and WORST >= MEAN, up to the one rounding of the division — one ulp of the larger side."""
    T, N = 8, 300
    rig = Rig("nav2d", T, N)
    grid = rig.solver._cost_owner._obstacle_map.grid_spec()
    cells, cell, origin = np.asarray(grid.cells), float(grid.cell_size), np.asarray(grid.origin, f64)
    occ = np.argwhere(cells[6:-6, 6:-6] > 0) + 6
    pick = next((ij for ij in occ if cells[ij[0] - 4, ij[1] - 4] == 0), None)
    assert pick is not None, "no obstacle cell with a free cell 0.4 m to its south-west"
    near = np.append((pick - 4 - origin) * cell, 0.785)
    parts = f32([near, [-9.0, -9.0, 0.785], [-8.5, -9.0, 0.785]])
    mean = np.broadcast_to(f32([1.5, 0.0]), (T, 2)).copy()
    rig.set_mean(mean)
    M, _ = particle_rows(rig, parts, 3)
    assert np.mean(M[0] > M[1] + 5000.0) > 0.2, "samples from the near particle hit the obstacle"
    out = {}
    for name, (mode, k) in dict(worst=("worst", 1), cvar2=("cvar", 2), cvar3=("cvar", 3), mean=("mean", 1)).items():
        risk(rig.h, mode, k)
        rig.h.call("mppi_set_particle_costs", M.ctypes.data_as(C.c_void_p), 0, stream())
        out[name] = costs_of(rig.h, N).astype(f64)

    def ge(a, b):
        return np.all(a + np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(f32)).astype(f64) >= b)

    assert ge(out["worst"], out["cvar2"]) and ge(out["cvar2"], out["cvar3"]) and ge(out["worst"], out["mean"])
    assert np.any(out["worst"] > out["mean"])
    rig.close()
