"""The opt-in features of the solve IN PAIRS on a real MI355X: every one of the 28 pairs of {control-cost term, correlated noise,
covariance adaptation, particles with a risk measure, exploration split, Savitzky-Golay step, device temperature rule,
sharding} as one closed loop of three ticks through the C ABI, against tests/solve_ref.py (the float64 restatement of a whole
tick composed from the single-feature references; tests/test_solve_ref_host.py anchors it and proves that every case here can
see the mistakes its pair could hide).  The case table — model, rule, shapes, temperatures — is solve_ref's.

Per tick, three handles of one configuration:
  a   the case itself: noise_regen = 1 and fused_solve = 1 asked for, whatever the features then admit;
  t   mppi_clone_state(a) BEFORE the tick, three times over:
        1. the other side of every path choice (noise_regen = 0, fused_solve = 0): the same tick, the same bits wherever both
           sides run the multi-kernel sequence, the same costs always;
        2. a probe for the costs: the math-level-0 identities (row m of the particle matrix == the plain rollout from
           particle m, costs == fold, costs == fold + kappa * A32, a window's costs == its part of the unsharded vector) and the
           costs of math levels 1 and 2 against float64 on the device's own U;
        3. the state round trip: the clone runs the tick with a's own options and must return a's bits.
Every quantity keeps the limit of its single-feature test (solve_ref.distances names them); every measured maximum goes to
parity_report.record.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import action_cost_ref as acref
import discs_ref as D
import emul
import mlp_ref as ML
import parity_report
import solve_ref as sr
import stats_cases as sc
import test_gpu_racing_discs as RAC
from helpers import rel_err, same_lbps_minimum
from pi_mpc import _host
from test_gpu_action_cost import Rig
from test_gpu_covariance import _need_gpu, check_table, make, weights64
from test_gpu_fused_geometry import took
from test_gpu_mlp_model import MlpRig
from test_gpu_noise_domain import pointwise_limit
from test_gpu_particles import matrix_of, put_particles, risk, same_bits, set_state, stream
from test_gpu_soft_discs import SoftNavRig

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
IDS = [sr.pair_id(p) for p in sr.PAIRS]
TOL = sr.TOL
SUM_TOL = 1e-5        # sum e of test_shard_invariance_and_combine; the sums of test_gpu_stats_geometry.py
SHARD_TOL = 2e-6      # action and states of two combined windows against the unsharded handle (test_shard_invariance_and_combine)
TILES_ONLY = {"CN", "CV"}        # mppi_handle.hpp::tiles_only
MULTI_KERNEL = {"AC", "PR", "CN", "CV"}  # capi_solve.hip::fused_applies declines (the term, the particles, no regenerated noise)
DRAW_PAIRS = [p for p in sr.PAIRS if set(p) == {"CN", "CV"} or (set(p) & {"CN", "CV"} and set(p) & {"SH", "EX"})]


def lam_device():
    from mppi_playground_amd import _capi

    return _capi.LAMBDA_DEVICE


# ------------------------------------------------------------------------------ rigs
def new_rig(pb, n=None):  # (pb: a Problem, or solve_ref.shape_of(pair): family, N, T and whether the split is on)
    """A native handle of the case's family with n samples (default: all N), math level 0; the exploration split rides in the
    configuration, every other feature is applied through the C ABI (apply)"""
    _need_gpu()
    T, N = pb.T, pb.N if n is None else n
    kw = dict(exploration=sr.EXPLORATION) if pb.inherit < pb.N else {}
    if pb.family == "nav_soft":
        table, x0 = D.case(sr.NAV_TABLE, T)
        rig = SoftNavRig(table, x0, None, T, N, setting=sr.SOFTNESS, math=0, **kw)
    elif pb.family == "racing_discs":
        table, x0, ref = RAC.case(sr.RACING_TABLE, T)
        rig = RAC.DiscRig(table, x0, ref, T, N, math=0, **kw)
    elif pb.family == "mlp42":
        rig = MlpRig(ML.case(sr.MLP_CASE), T, N, math=0, **kw)
    else:
        rig = Rig(pb.family, T, N, **kw)
        rig.h.call("mppi_set_option", b"math", 0)
    return rig


def model_of(rig, family):
    if family == "nav_soft":
        return sr.SoftNavModel(rig.P, rig.grid, rig.table, *sr.SOFTNESS)
    if family == "racing_discs":
        return sr.RacingDiscModel(rig.P, rig.grids, rig.ref_path, rig.table)
    if family == "mlp42":
        return sr.MlpModel(rig.cs)
    return sr.OracleModel(family)


def rewindow(rig, pb, offset, n):
    """Re-create the rig's handle as the n samples from GLOBAL index `offset` on, of pb.N (a shard of the problem)"""
    from mppi_playground_amd import _capi

    sol = rig.solver
    cfg = _capi.MppiConfig()
    cfg.model = _capi.MODEL_IDS[sol._model]
    cfg.horizon, cfg.dim_state, cfg.dim_control = pb.T, pb.ds, pb.dc
    cfg.num_samples, cfg.sample_offset, cfg.inherit_count = n, int(offset), int(pb.inherit)
    for k in range(pb.dc):
        cfg.u_min[k], cfg.u_max[k], cfg.sigmas[k] = float(pb.u_min[k]), float(pb.u_max[k]), float(pb.sigmas[k])
    cfg.seed, cfg.device = sol._seed, 0
    sol._h.close()
    sol._h = _capi.Handle(cfg)
    sol._uploaded, sol._params_set, sol._ref_uploaded = {}, None, None
    rig.N = n
    rig._prepare()
    rig.h.call("mppi_set_option", b"math", 0)


def apply(rig, pb):
    """Every feature of the problem that a handle holds, through the C ABI"""
    from mppi_playground_amd import _capi

    h = rig.h
    fl = lambda a: (C.c_float * pb.dc)(*[float(v) for v in a])  # noqa: E731
    if pb.ac_weight is not None:
        h.call("mppi_set_action_cost", 1, float(pb.ac_weight))
    if pb.beta is not None:
        h.call("mppi_set_noise_correlation", fl(pb.beta))
    if pb.cov is not None:
        h.call("mppi_set_covariance_adaptation", 1, pb.cov["rate"], pb.cov["floor"], fl(pb.cov["smin"]), fl(pb.cov["smax"]))
    if pb.sg is not None:
        h.call("mppi_set_sg_filter", pb.sg.ctypes.data_as(C.c_void_p), int(len(pb.sg)), None)
    if pb.rule is not None:
        p, lo, hi = pb.rule_args()
        if pb.rule == "MPO":
            h.call("mppi_mpo_reset", float(pb.lams[0]), sr.MPO_EPS, sr.MPO_LR)
            h.call("mppi_set_auto_lambda", _capi.AUTO_RULES["MPO"], 0.0, 0.0, 0.0)
        else:
            if pb.rule.startswith("LBPS"):
                h.call("mppi_set_option", b"lbps_search", 1 if pb.rule == "LBPS_GRID" else 0)
            h.call("mppi_set_auto_lambda", _capi.AUTO_RULES[pb.rule[:5].rstrip("_")], float(p), float(lo), float(hi))
    rig.set_mean(pb.mean0())


def clone(dst, src):
    dst.h.call("mppi_clone_state", src.h.h)


def sigma_of(rig):
    t = torch.empty(rig.T, rig.dc, device="cuda")
    rig.h.call("mppi_get_sigma_table", t.data_ptr(), 1, stream())
    return t.cpu().numpy()


def set_sigma(rig, table):
    rig._sig_keep = torch.from_numpy(np.ascontiguousarray(table, f32)).cuda()
    rig.h.call("mppi_set_sigma_table", rig._sig_keep.data_ptr(), 1, stream())


def hist_of(rig):
    out = np.empty((rig.T - 1, rig.dc), f32)
    rig.h.call("mppi_get_sg_history", out.ctypes.data_as(C.c_void_p))
    return out


def lambdas_of(rig):
    nxt, used = C.c_double(0.0), C.c_double(0.0)
    rig.h.call("mppi_get_lambda", C.byref(nxt), C.byref(used), stream())
    return nxt.value, used.value


def mpo_state(rig):
    st4 = (C.c_double * 4)()
    rig.h.call("mppi_mpo_state", st4)
    return np.array(list(st4), f64)


def noise_of(rig):
    e = torch.empty(rig.N, rig.T, rig.dc, device="cuda")
    rig.h.call("mppi_export_noise", e.data_ptr(), None, stream())
    return e.cpu().numpy()


def states_of(rig):
    idx = torch.arange(rig.N, device="cuda", dtype=torch.int64)
    out = torch.empty(rig.N, rig.T + 1, rig.ds, device="cuda")
    rig.h.call("mppi_rollout_samples", idx.data_ptr(), rig.N, out.data_ptr(), stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def top_of(rig, k, lam):
    st, w = torch.empty(k, rig.T + 1, rig.ds, device="cuda"), torch.empty(k, device="cuda")
    rig.h.call("mppi_top_samples", k, float(lam), st.data_ptr(), w.data_ptr(), stream())
    torch.cuda.synchronize()
    return st.cpu().numpy(), w.cpu().numpy()


def before(rig, pb, tick, x, prev_lam):
    """The carry of solve_ref.tick as the handle holds it before a tick"""
    tl = None
    if pb.rule == "MPO":
        tl = dict(mpo=mpo_state(rig), lam=lambdas_of(rig)[0])  # (the temperature in force: what the dual left on the device)
    elif pb.rule is not None:
        tl = dict(prev=prev_lam)
    return dict(t=tick, x=f32(x), mean=rig.mean(), sigma=sigma_of(rig), hist=hist_of(rig) if pb.sg is not None else None, tl=tl)


def prepare(rig, pb, x):
    set_state(rig, x)
    parts = pb.particles(x)
    if parts is not None:
        put_particles(rig.h, parts, on_device=True)
        risk(rig.h, *pb.risk)
    return parts


def run_tick(rig, pb, carry, idx):
    """One mppi_solve of the case on `rig` -> everything the tick left, as numpy"""
    parts = prepare(rig, pb, carry["x"])
    lam_arg = lam_device() if pb.rule is not None else pb.lams[carry["t"]]
    action, states, stats, costs = rig.solve(idx, lam_arg)
    rec = dict(action=action, states=states, stats=stats, costs=costs, took=took(rig.h), lam_arg=lam_arg)
    rec["lambda_next"], rec["lambda"] = lambdas_of(rig) if pb.rule is not None else (lam_arg, lam_arg)
    rec["matrix"] = matrix_of(rig.h, len(parts), rig.N) if parts is not None else None
    rec["eps"] = noise_of(rig)
    rec["U"] = rig.actions_around(carry["mean"])
    rec["sigma"], rec["mean"] = sigma_of(rig), rig.mean()
    rec["hist"] = hist_of(rig) if pb.sg is not None else None
    rec["top"] = top_of(rig, 4, rec["lambda"])
    rec["mpo"] = mpo_state(rig) if pb.rule == "MPO" else None
    return rec


def record(quantity, value, limit, **extra):
    parity_report.record("pairs_" + quantity, value, limit, **extra)


# ------------------------------------------------------------------------------ one tick against the restatement
def check_temperature(name, pb, carry, rec, rig):
    """The device's temperature against the host search (tests/emul.py, through solve_ref.temperature) on the device's final
    costs, at the limits of test_gpu_stats_geometry.py"""
    if pb.rule is None:
        return
    lam, c = rec["lambda"], rec["costs"]
    want, _, nxt = sr.temperature(pb, carry["tl"], c, carry["t"])
    p, lo, hi = pb.rule_args()
    err = abs(lam - want) / want
    print(f"[pairs] {name}: temperature {lam:.9g} against the host search's {want:.9g} (rel {err:.3e}), rule {pb.rule}")
    if pb.rule == "ESSPS":
        record("essps_vs_host_search", err, sc.WARM_TOL)
        assert err <= sc.WARM_TOL, (name, lam, want)
        off = abs(weights64(c, lam)[1] - p) / p
        record("essps_ess64", off, sc.ESS_BAND)
        assert lo < lam < hi and off <= sc.ESS_BAND, (name, lam, off)
    elif pb.rule.startswith("LBPS"):
        assert same_lbps_minimum(c, lam, want, delta=p), (name, lam, want)
    else:  # MPO: this tick's weights use the dual's temperature before its step; the step itself is held from the device's sums
        assert abs(lam - want) <= 2e-6 * want, (name, lam, want)
        st5 = (C.c_double * 5)()
        rig.h.call("mppi_softmax_stats", C.c_float(float(sc.softplus32(carry["tl"]["mpo"][0]))), st5, stream())
        state, lam_next = emul.mpo_step_stats(carry["tl"]["mpo"], sr.MPO_EPS, sr.MPO_LR, list(st5))
        ulp = max(sc.ulp32(rec["mpo"][i], state[i]) for i in range(3))
        print(f"[pairs] {name}: the dual's step within {ulp:.2f} fp32 ulp of the host step on the device's sums (limit {sc.MPO_ULP})")
        assert rec["mpo"][3] == state[3] and ulp <= sc.MPO_ULP, (name, rec["mpo"], state)
        assert abs(rec["lambda_next"] - lam_next) <= 2e-6 * lam_next, (name, rec["lambda_next"], lam_next)


def check_tick(name, pb, carry, rec, rig):
    """Everything a tick left on the device against solve_ref.tick on the device's own noise, U, costs and temperature"""
    check_temperature(name, pb, carry, rec, rig)
    parts = pb.particles(carry["x"])
    # (the soft model's float64 costs are judged on the device's own states; with particles there is one set per particle, which
    # probe_costs collects: here the level-0 costs of such a case are held by the identities alone)
    judged = not (pb.model.own_states and parts is not None)
    states = states_of(rig) if (pb.model.own_states and parts is None) else None
    ref = sr.tick(pb, carry, rec["eps"], given=dict(U=rec["U"], costs=rec["costs"], **{"lambda": rec["lambda"]}), states=states)
    lam = rec["lambda"]
    assert np.all(np.isfinite(rec["costs"])) and np.all(np.isfinite(rec["action"])) and np.all(np.isfinite(rec["states"])), name
    # U is clamp(mean_i + eps) with the inherit test on the GLOBAL index
    same_bits(f"{name}: U", rec["U"], ref["U_ref"])
    # costs (math level 0 here): the model's own limit, boundary samples within the cap
    if judged:
        worst, left = sr.cost_excess(rec["costs"], dict(ref, limit=pb.model.limit))
        record("costs_level0_of_limit", worst, 1.0, left_out=left)
        assert left <= sr.boundary_cap(pb.n), f"{name}: {left} boundary samples"
        assert worst <= 1.0, f"{name}: costs {worst:.3g} of their limit"
    # the summary {min, sum e, sum e^2, sum e*c}
    st, want = rec["stats"].astype(f64), ref["stats"]
    same_bits(f"{name}: minimum", [rec["stats"][0]], [rec["costs"].min()])
    errs = [abs(st[1] - want[1]) / want[1], abs(st[2] - want[2]) / want[2], abs(st[3] - want[3]) / ref["abs_ec"]]
    record("summary_sums", max(errs), SUM_TOL)
    assert max(errs) <= SUM_TOL, (name, st, want)
    # the action, the state sequence from the NOMINAL state, the warm start
    err_a = rel_err(rec["action"], ref["action"])
    err_s = rel_err(rec["states"], pb.model.single(carry["x"], rec["action"]))
    record("action_rel_err", err_a, TOL)
    record("state_rel_err", err_s, TOL)
    assert err_a < TOL and err_s < TOL, (name, err_a, err_s)
    same_bits(f"{name}: state_seq[0] is the nominal state", rec["states"][0], carry["x"])
    same_bits(f"{name}: the warm start is the action", rec["mean"], rec["action"])
    # the filter history
    if pb.sg is not None:
        same_bits(f"{name}: history", rec["hist"], np.concatenate([carry["hist"][1:], rec["action"][:1]]))
        err_h = float(np.abs(rec["hist"] - ref["hist"]).max() / max(np.abs(ref["action"]).max(), 1e-30))
        record("history_rel_err", err_h, TOL)
        assert err_h < TOL, (name, err_h)
    # the sigma table after the step: test_gpu_covariance.check_table, as it stands, on the device's own U and costs
    if pb.cov is not None:
        cv = pb.cov
        check_table(name, rec["sigma"], rec["U"], rec["costs"], lam, carry["sigma"], rate=cv["rate"], floor=cv["floor"],
                    smin=cv["smin"], smax=cv["smax"])
        err_t = float(np.max(np.abs(rec["sigma"].astype(f64) - ref["sigma"]) / ref["sigma"]))
        record("sigma_rel_err", err_t, TOL)
    else:
        same_bits(f"{name}: the sigma table stays", rec["sigma"], carry["sigma"])
    # the four best samples: states re-rolled from the nominal state, weights
    top_s, top_w = rec["top"]
    five = np.sort(rec["costs"])[:5]
    if len(np.unique(five)) == 5:  # (no tie around the cut: the order is determined)
        err_ts, err_tw = rel_err(top_s, ref["top_states"]), rel_err(top_w, ref["top_weights"])
        record("top_states_rel_err", err_ts, TOL)
        record("top_weights_rel_err", err_tw, TOL)
        assert err_ts < TOL and err_tw < TOL, (name, err_ts, err_tw)
    same_bits(f"{name}: top samples start at the nominal state", top_s[:, 0, :], np.broadcast_to(f32(carry["x"]), (4, pb.ds)))
    return ref


def check_draw(name, pb, carry, eps, idx, offset=0):
    """The exported noise against the restated draw: normals at the GLOBAL index, the filter, the per-step sigma"""
    n = eps.shape[0]
    want = sr.draw(idx, offset, n, pb.T, pb.dc, pb.beta, carry["sigma"])
    lim = sr.draw_bound(pb.beta, carry["sigma"], pb.T, pb.dc, pointwise_limit())
    worst = float(np.max(np.abs(eps.astype(f64) - want) / lim[None]))
    record("draw_of_bound", worst, 1.0)
    print(f"[pairs] {name}: exported noise within {worst:.3g} of its bound against the restated draw")
    assert worst <= 1.0, (name, worst)


def same_record(name, a, b, tail):
    """Two sides of a path choice: the costs always, the tail wherever both ran the multi-kernel sequence"""
    same_bits(f"{name}: costs", a["costs"], b["costs"])
    same_bits(f"{name}: U", a["U"], b["U"])
    same_bits(f"{name}: noise", a["eps"], b["eps"])
    if a["matrix"] is not None:
        same_bits(f"{name}: matrix", a["matrix"], b["matrix"])
    if tail:
        for key in ("action", "states", "stats", "sigma", "mean"):
            same_bits(f"{name}: {key}", a[key], b[key])
        if a["hist"] is not None:
            same_bits(f"{name}: history", a["hist"], b["hist"])
        assert a["lambda"] == b["lambda"] and a["lambda_next"] == b["lambda_next"], (name, a["lambda"], b["lambda"])
        same_bits(f"{name}: top states", a["top"][0], b["top"][0])
        same_bits(f"{name}: top weights", a["top"][1], b["top"][1])


# ------------------------------------------------------------------------------ the probe: identities at level 0, levels 1 and 2
def probe_costs(name, t, pb, carry, idx, rec):
    """`t` holds a's state before the tick.  Math level 0: the identities, bit for bit.  Levels 1 and 2: the costs against
    float64 on the device's own U (and, for the soft model, the device's own states)."""
    h = t.h
    parts = pb.particles(carry["x"])
    lam_term = sr.term_lambda(pb, carry["tl"], carry["t"])
    U = rec["U"]
    # ---- level 0
    folded = rec["costs"]
    if parts is not None:
        h.call("mppi_set_particles", None, 0, 0, stream())
        if pb.ac_weight is not None:
            h.call("mppi_set_action_cost", 1, 0.0)
        for m, x in enumerate(parts):
            set_state(t, x)
            same_bits(f"{name}: row {m} is the plain rollout from particle {m}", rec["matrix"][m], t.rollout(idx))
        folded = _host.fold_particle_costs(rec["matrix"], *pb.risk)
        if pb.ac_weight is None:
            same_bits(f"{name}: costs are the fold of the matrix", rec["costs"], folded)
    if pb.ac_weight is not None:
        if parts is None:
            set_state(t, carry["x"])
            h.call("mppi_set_action_cost", 1, 0.0)
            folded = t.rollout(idx)
        g = acref.g32(carry["mean"], carry["sigma"])
        kappa = acref.kappa32(pb.ac_weight, lam_term)
        acref.check(name, rec["costs"], folded, kappa, g, U)
        same_bits(f"{name}: costs are total32(folded, kappa, A32)", rec["costs"], acref.total32(folded, kappa, acref.A32(g, U)))
        h.call("mppi_set_action_cost", 1, float(pb.ac_weight))
    # ---- levels 1 and 2, with every feature of the case on again
    prepare(t, pb, carry["x"])
    if pb.ac_weight is not None:
        h.call("mppi_set_action_cost_lambda", float(rec["lam_arg"]))
    for level in (1, 2):
        h.call("mppi_set_option", b"math", level)
        c = t.rollout(idx)
        M = matrix_of(h, len(parts), t.N) if parts is not None else None
        Ul = t.actions_around(carry["mean"])
        same_bits(f"{name} math {level}: U", Ul, U)
        states = None
        if pb.model.own_states:
            if parts is None:
                states = states_of(t)
            else:  # (the re-roll starts at the nominal state: one plain rollout per particle gives that particle's states)
                states = []
                h.call("mppi_set_particles", None, 0, 0, stream())
                for x in parts:
                    set_state(t, x)
                    t.rollout(idx)
                    states.append(states_of(t))
                prepare(t, pb, carry["x"])
        ref = sr.tick(pb, carry, rec["eps"], given=dict(U=Ul), states=states)
        worst, left = sr.cost_excess(c, dict(ref, limit=pb.model.limit))
        record(f"costs_level{level}_of_limit", worst, 1.0, left_out=left)
        print(f"[pairs] {name} math {level}: costs {worst:.3g} of their limit, {left} boundary samples left out (cap {sr.boundary_cap(pb.n)})")
        assert np.all(np.isfinite(c)), name
        assert left <= sr.boundary_cap(pb.n), f"{name} math {level}: {left} boundary samples"
        assert worst <= 1.0, f"{name} math {level}: costs {worst:.3g} of their limit"
        if M is not None and pb.ac_weight is None:  # the fold of the fast rows is the fold
            same_bits(f"{name} math {level}: fold", c, _host.fold_particle_costs(M, *pb.risk))
    h.call("mppi_set_option", b"math", 0)


# ------------------------------------------------------------------------------ the sharded side
def sharded_tick(name, halves, pb, carry, idx, rec):
    """Two windows of the global samples (sample_offset 0 and N / 2) on handles of their own: the unsharded handle's noise and
    costs part for part, bit for bit; combined by mppi_finalize(num_shards = 2): the unsharded plan."""
    n = pb.N // 2
    lam = float(rec["lambda"])
    sums, outs = [], []
    for r, hf in enumerate(halves):
        w = pb.window(r * n, n)
        parts = prepare(hf, w, carry["x"])
        hf.set_mean(carry["mean"])
        if pb.cov is not None:
            set_sigma(hf, carry["sigma"])
        if pb.sg is not None:  # (every rank filters with the history it kept: the same one)
            hf.h.call("mppi_set_sg_filter", pb.sg.ctypes.data_as(C.c_void_p), int(len(pb.sg)), carry["hist"].ctypes.data_as(C.c_void_p))
        if pb.ac_weight is not None:
            hf.h.call("mppi_set_action_cost_lambda", float(sr.term_lambda(pb, carry["tl"], carry["t"])))
        c = hf.rollout(idx)
        eps = noise_of(hf)
        same_bits(f"{name} window {r}: noise", eps, rec["eps"][r * n:(r + 1) * n])
        same_bits(f"{name} window {r}: U", hf.actions_around(carry["mean"]), rec["U"][r * n:(r + 1) * n])
        same_bits(f"{name} window {r}: costs", c, rec["costs"][r * n:(r + 1) * n])
        if parts is not None:
            same_bits(f"{name} window {r}: matrix", matrix_of(hf.h, len(parts), n), rec["matrix"][:, r * n:(r + 1) * n])
        if pb.pair in DRAW_PAIRS:
            check_draw(f"{name} window {r}", w, carry, eps, idx, offset=r * n)
        s = torch.zeros(4 + pb.T * pb.dc, device="cuda")
        hf.h.call("mppi_weights_reduce", lam, C.c_void_p(s.data_ptr()), stream())
        sums.append(s)
    both = torch.stack(sums).contiguous()
    for r, hf in enumerate(halves):
        hf.action.fill_(float("nan")), hf.state.fill_(float("nan")), hf.stats.fill_(float("nan"))
        hf.h.call("mppi_finalize", C.c_void_p(both.data_ptr()), 2, lam, 1, hf.action.data_ptr(), hf.state.data_ptr(),
                  hf.stats.data_ptr(), stream())
        hf.h.call("mppi_join_state_seq", 0, stream())
        torch.cuda.synchronize()
        outs.append((hf.action.cpu().numpy(), hf.state.cpu().numpy()[0], hf.stats.cpu().numpy(), hf.mean()))
    for key, (p, q) in zip(("action", "states", "stats", "warm start"), zip(*outs)):
        same_bits(f"{name}: both ranks hold the same {key}", p, q)
    act, sts, st, _ = outs[0]
    ea, es = rel_err(act, rec["action"]), rel_err(sts, rec["states"])
    record("shard_action_vs_unsharded", ea, SHARD_TOL)
    record("shard_states_vs_unsharded", es, SHARD_TOL)
    print(f"[pairs] {name}: two windows against the unsharded handle: action {ea:.3g}, states {es:.3g}")
    assert ea < SHARD_TOL and es < SHARD_TOL, (name, ea, es)
    assert st[0] == rec["stats"][0] and abs(st[1] - rec["stats"][1]) <= SUM_TOL * rec["stats"][1], (name, st, rec["stats"])
    # ... and against the restatement of the two windows (tick_sharded's combined tail on the windows' own U and costs)
    ref = sr.tick(pb, carry, rec["eps"], given=dict(U=rec["U"], costs=rec["costs"], **{"lambda": lam}))
    err = rel_err(act, ref["action"])
    record("shard_action_rel_err", err, TOL)
    assert err < TOL, (name, err)
    if pb.sg is not None:
        same_bits(f"{name}: the ranks' history", hist_of(halves[0]), hist_of(halves[1]))


# ------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("pair", sr.PAIRS, ids=IDS)
def test_pair(pair):
    shape = sr.shape_of(pair)
    first_entry = len(parity_report.entries)
    a = new_rig(shape)
    pb = sr.Problem(pair, model_of(a, shape.family), a.x0.cpu().numpy())
    assert (pb.N, pb.T, pb.dc, pb.ds) == (a.N, a.T, a.dc, a.ds)
    t = new_rig(pb)
    for rig in (a, t):
        apply(rig, pb)
    halves = []
    if "SH" in pair:
        for r in range(2):
            hf = new_rig(pb, pb.N // 2)
            rewindow(hf, pb, r * (pb.N // 2), pb.N // 2)
            apply(hf, pb)
            halves.append(hf)
    multi = bool(set(pair) & MULTI_KERNEL) or pb.rule == "LBPS_BRENT"  # (the single launch searches LBPS on grids only)
    a.h.call("mppi_set_option", b"noise_regen", 1)
    a.h.call("mppi_set_option", b"fused_solve", 1)
    x, prev_lam, seen = a.x0.cpu().numpy(), 0.0, []
    for tick in range(sr.TICKS):
        idx = tick + 1
        name = f"{sr.pair_id(pair)} tick {tick}"
        carry = before(a, pb, tick, x, prev_lam)
        # 1. the other side of every path choice, from a's state before the tick
        clone(t, a)
        t.h.call("mppi_set_option", b"noise_regen", 0)
        t.h.call("mppi_set_option", b"fused_solve", 0)
        other = run_tick(t, pb, carry, idx)
        assert other["took"] == (0, 0), name
        check_tick(name + " (tiles, multi-kernel)", pb, carry, other, t)
        # 2. the state round trip, once warm start, history, sigma table, dual and minimum slot have all carried over: the
        # clone runs the tick with a's own options
        trip = None
        if tick == sr.TICKS - 1:
            clone(t, a)
            trip = run_tick(t, pb, carry, idx)
        # 3. the probe: a's state before the tick once more (the twin's costs, U and matrix are a's, bit for bit: below)
        clone(t, a)
        probe_costs(name, t, pb, carry, idx, other)
        # 4. the case itself
        rec = run_tick(a, pb, carry, idx)
        if multi:
            assert rec["took"] == (0, 0), f"{name}: {pair} must decline the single launch, took {rec['took']}"
        else:
            assert rec["took"] != (0, 0), f"{name}: the single launch applies to {pair}"
            assert a.h.lib.mppi_fused_error(a.h.h) == 0, name
        check_tick(name, pb, carry, rec, a)
        same_record(name + ": the two sides", rec, other, tail=multi)
        if trip is not None:
            assert trip["took"] == rec["took"], name
            same_record(name + ": the clone", trip, rec, tail=True)
        if pair in DRAW_PAIRS:
            check_draw(name, pb, carry, rec["eps"], idx)
        if halves:
            sharded_tick(name, halves, pb, carry, idx, rec)
        seen.append(rec)
        x, prev_lam = rec["states"][1].copy(), rec["lambda"]
    assert not np.array_equal(seen[0]["action"], seen[-1]["action"]), "the closed loop moved"
    worst = {}
    for e in parity_report.entries[first_entry:]:
        if e["value"] >= worst.get(e["quantity"], (-1.0, 0.0))[0]:
            worst[e["quantity"]] = (e["value"], e["limit"])
    paths = ("multi-kernel (single launch declined)" if multi else "single launch %s" % (seen[-1]["took"],)) + " + multi-kernel twin; noise regenerated" + \
        (" asked, tiles taken" if set(pair) & TILES_ONLY else "") + " + tiles twin" + ("; two windows + mppi_finalize(2)" if halves else "")
    print(f"[pairs] SUMMARY | {sr.pair_id(pair)} | {pb.family} | {pb.rule or 'fixed'} | {paths} | " +
          "; ".join(f"{q[6:]} {v:.3g} / {lim:.3g}" for q, (v, lim) in sorted(worst.items())))
    if pb.cov is not None:
        assert not np.array_equal(seen[-1]["sigma"], np.tile(pb.sigmas, (pb.T, 1)))
    for rig in [a, t] + halves:
        rig.close()


# ------------------------------------------------------------------------------ through pi_mpc.mppi.MPPI
SOLVER_FEATURES = ("AC", "CN", "CV", "PR", "EX", "SG", "TL")   # what the constructor and the setters expose (SH needs ranks)
SOLVER_PAIRS = [p for p in sr.PAIRS if set(p) <= set(SOLVER_FEATURES) and set(p) != {"AC", "CN"}]  # (that one is refused: below)


def solver_kwargs(pb):
    kw = {}
    if pb.ac_weight is not None:
        kw.update(action_cost=True, action_cost_weight=pb.ac_weight)
    if pb.beta is not None:
        kw.update(noise_beta=torch.from_numpy(pb.beta.copy()))
    if pb.cov is not None:
        kw.update(adapt_covariance=True, cov_rate=pb.cov["rate"], cov_floor=pb.cov["floor"], sigma_min=torch.from_numpy(pb.cov["smin"]),
                  sigma_max=torch.from_numpy(pb.cov["smax"]))
    if "PR" in pb.on:
        kw.update(risk=pb.risk[0], risk_alpha=0.5)   # ceil(0.5 * 3) = 2 of 3 particles under CVaR
    if "EX" in pb.on:
        kw.update(exploration=sr.EXPLORATION)
    if pb.sg is not None:
        kw.update(use_sg_filter=True, sg_window_size=len(pb.sg), sg_poly_order=3)
    if pb.rule is not None:
        p, lo, hi = pb.rule_args()
        kw.update(essps_target_ess=p, lambda_min=lo, lambda_max=hi)
    return kw


def solver_case(pair):
    pb = sr.Problem(pair, sr.OracleModel("pendulum"), [3.0, 0.1], family="pendulum")
    pb.lams = (1.0, 1.0, 1.0)
    if "TL" in pair:
        pb.rule = "ESSPS"
    build = lambda: make("pendulum", pb.T, pb.N, "ESSPS" if "TL" in pair else 1.0, **solver_kwargs(pb))  # noqa: E731
    solver, x0 = build()
    assert (pb.N, pb.T, pb.inherit) == (200, 7, 140 if "EX" in pair else 200)
    solver.set_warm_start(pb.mean0())
    return pb, solver, x0.cuda(), build


def solver_tick(pb, solver, x, pair):
    if "PR" in pair:
        solver.set_state_particles(torch.from_numpy(pb.particles(x.cpu().numpy())).cuda())
    return solver.forward(x)


@pytest.mark.parametrize("pair", SOLVER_PAIRS, ids=[sr.pair_id(p) for p in SOLVER_PAIRS])
def test_solver_hands_both_settings_to_the_handle(pair):
    """Two ticks of pi_mpc.mppi.MPPI (pendulum) with both options given to the constructor or the setters: the action and
    last_stats() against the restatement on the solver's own noise, U and costs"""
    from test_gpu_action_cost import current_mean

    pb, solver, x, _ = solver_case(pair)
    prev = 0.0
    for tick in range(2):
        name = f"solver {sr.pair_id(pair)} tick {tick}"
        carry = dict(t=tick, x=x.cpu().numpy(), mean=current_mean(solver), sigma=solver.sigma_seq.cpu().numpy(),
                     hist=np.array(solver._actions_history_for_sg, copy=True) if pb.sg is not None else None,
                     tl=dict(prev=prev) if pb.rule else None)
        a, s = solver_tick(pb, solver, x, pair)
        assert (took(solver._h) == (0, 0)) == bool(set(pair) & MULTI_KERNEL), (name, took(solver._h))
        lam = float(solver._last_lambda)
        costs, U, eps = solver._costs.cpu().numpy(), solver._perturbed_action_seqs.cpu().numpy(), solver._action_noises.cpu().numpy()
        if pb.rule:
            want = sr.temperature(pb, carry["tl"], costs, tick)[0]
            record("solver_essps_vs_host_search", abs(lam - want) / want, sc.WARM_TOL)
            assert abs(lam - want) <= sc.WARM_TOL * want, (name, lam, want)
        ref = sr.tick(pb, carry, eps, given=dict(U=U, costs=costs, **{"lambda": lam}))
        same_bits(f"{name}: U", U, ref["U_ref"])
        worst, left = sr.cost_excess(costs, dict(ref, limit=pb.model.limit))
        record("solver_costs_of_limit", worst, 1.0)
        assert worst <= 1.0 and left == 0, (name, worst, left)
        err = rel_err(a.cpu().numpy(), ref["action"])
        record("solver_action_rel_err", err, TOL)
        assert err < TOL, (name, err)
        st = solver.last_stats()
        assert st["cmin"] == costs.min() and st["lambda_"] == lam, (name, st)
        got, want = [st["sum_e"], st["sum_e2"], st["sum_ec"]], ref["stats"][1:]
        errs = [abs(got[0] - want[0]) / want[0], abs(got[1] - want[1]) / want[1], abs(got[2] - want[2]) / ref["abs_ec"]]
        record("solver_summary_sums", max(errs), SUM_TOL)
        assert max(errs) <= SUM_TOL, (name, got, want)
        if pb.cov is not None:
            cv = pb.cov
            check_table(name, solver.sigma_seq.cpu().numpy(), U, costs, lam, carry["sigma"], rate=cv["rate"], floor=cv["floor"],
                        smin=cv["smin"], smax=cv["smax"])
        if "PR" in pair and pb.ac_weight is None:
            same_bits(f"{name}: fold", costs, _host.fold_particle_costs(solver.particle_costs.cpu().numpy(), *pb.risk))
        x, prev = s[0, 1].clone(), lam


@pytest.mark.parametrize("pair", SOLVER_PAIRS, ids=[sr.pair_id(p) for p in SOLVER_PAIRS])
def test_solver_state_dict_round_trip(pair):
    """After two ticks a fresh solver loads this one's state_dict(); both must produce the third tick bit for bit.

    Two things this test found are fixed with it.  With the control-cost term and a search on the device (ACxTL) the restored
    handle held no temperature, the term got a zero factor for one solve and the plan came back different altogether
    (pi_mpc/_module.py::set_extra_state puts the temperature back).  And state_dict() did not carry the warm start of the
    device-resident ESSPS search (EsspsDev: the first grid the last search left behind), so every restored TL solver searched from
    the cold grid and found its temperature 3e-8 to 1.2e-6 away, actions up to 1.9e-6: mppi_essps_get_state / _set_state carry
    it now."""
    pb, solver, x, build = solver_case(pair)
    for _ in range(2):
        a, s = solver_tick(pb, solver, x, pair)
        x = s[0, 1].clone()
    fresh, _ = build()
    fresh.load_state_dict(solver.state_dict())
    outs = []
    for sol in (solver, fresh):
        a, s = solver_tick(pb, sol, x, pair)
        outs.append((sol._costs.clone(), sol._action_noises.clone(), a.clone(), s.clone(), sol.sigma_seq.clone(),
                     float(sol._last_lambda), took(sol._h)))
    dl = abs(outs[0][5] - outs[1][5]) / outs[0][5]
    print(f"[pairs] solver {sr.pair_id(pair)} after the state_dict round trip: temperature {outs[0][5]:.9g} against {outs[1][5]:.9g} "
          f"(rel {dl:.2e}), action {rel_err(outs[1][2].cpu().numpy(), outs[0][2].cpu().numpy()):.2e} apart")
    for key, p, q in zip(("costs", "noise", "action", "states", "sigma table"), outs[0], outs[1]):
        assert torch.equal(p, q), f"solver {sr.pair_id(pair)}: {key} after the state_dict round trip"
    assert outs[0][5:] == outs[1][5:], (pair, outs[0][5:], outs[1][5:])


# ------------------------------------------------------------------------------ the pairs the library refuses
def refused(rig, exc, match, call):
    """The call is refused with its message and leaves costs, mean and sigma table as they were"""
    keep = rig.costs(), rig.mean(), sigma_of(rig)
    with pytest.raises(exc, match=match):
        call()
    for name, was, now in zip(("costs", "mean", "sigma table"), keep, (rig.costs(), rig.mean(), sigma_of(rig))):
        same_bits(f"after the refusal: {name}", now, was)


def test_refused_pairs():
    from mppi_playground_amd._capi import MppiError

    rig = Rig("pendulum", 7, 200)
    rig.set_mean(np.linspace(-1.0, 1.0, 7, dtype=f32))
    rig.rollout(1)
    h = rig.h
    parts = f32([[3.0, 0.1], [3.1, 0.0], [2.9, 0.2]])
    # mapping = 1 (a wavefront per trajectory) with particles or with the term, whichever comes first
    put_particles(h, parts)
    refused(rig, MppiError, "particles are not available with mapping = 1", lambda: h.call("mppi_set_option", b"mapping", 1))
    h.call("mppi_set_particles", None, 0, 0, stream())
    h.call("mppi_set_action_cost", 1, 1.0)
    refused(rig, MppiError, "control-cost term is not available with mapping = 1", lambda: h.call("mppi_set_option", b"mapping", 1))
    h.call("mppi_set_action_cost", 0, 1.0)
    h.call("mppi_set_option", b"mapping", 1)
    refused(rig, MppiError, "particles are not available with mapping = 1", lambda: put_particles(h, parts))
    refused(rig, MppiError, "control-cost term is not available with mapping = 1", lambda: h.call("mppi_set_action_cost", 1, 1.0))
    h.call("mppi_set_option", b"mapping", 0)
    # covariance adaptation on a handle whose summaries travel between ranks (the variance would need a second exchange)
    h.call("mppi_set_covariance_adaptation", 1, 0.5, 1e-4, None, None)
    for key in (b"exchange_comm", b"exchange_p2p"):
        refused(rig, MppiError, "covariance adaptation is not available for sharded solves", lambda: h.call("mppi_set_option", key, 1))
    rig.close()
    # ... and what the Python solver rejects before a handle exists
    with pytest.raises(ValueError, match="shard_samples"):
        make("pendulum", 7, 200, 1.0, adapt_covariance=True, shard_samples=True)
    with pytest.raises(ValueError, match="action_cost"):
        make("pendulum", 7, 200, 1.0, action_cost=True, noise_beta=0.5)
    solver, x0 = make("pendulum", 7, 200, 1.0, action_cost=True)
    solver.forward(x0.cuda())
    keep = solver._costs.clone(), solver._previous_action_seq.clone(), solver.sigma_seq.clone()
    with pytest.raises(ValueError, match="action_cost"):
        solver.set_noise_beta(0.5)
    assert torch.equal(solver._costs, keep[0]) and torch.equal(solver._previous_action_seq, keep[1]) and torch.equal(solver.sigma_seq, keep[2])
    assert not solver.noise_beta.any()
