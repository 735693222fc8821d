"""One float64 restatement of a whole solver tick, COMPOSED from the references the suite already holds, and the table of
feature-pair cases that tests/test_solve_ref_host.py (CPU) and tests/test_gpu_feature_pairs.py (MI355X) share.

Nothing is derived a second time here.  The pieces and their owners:
  rollout + cost     discs_ref / soft_discs_ref / racing_discs_ref / mlp_ref (all take `dtype`), the oracle behind
                     helpers.oracle_problem for the shipped models (fp32: it IS the yardstick of test_gpu_parity.check_costs)
  particle fold      pi_mpc._host.fold_particle_costs (fp32, the header's order) and particle_cases.fold64
  control-cost term  action_cost_ref: g32, A32 / A64, kappa32, total32 — added BEHIND the fold, g from the sigma table in force
  weights            test_gpu_covariance.weights64: the fp32 argument the kernels form, exp and everything after in float64
  weighted mean      the expression of test_gpu_covariance.restate / test_gpu_action_cost.softmax_action
  filter             pi_mpc._host.sg_filter_sequence (the fp32 host statement the device equals bit for bit)
  sigma table        test_gpu_covariance.restate (float64) and test_covariance_host.numpy_step (fp32): the second moment is
                     centred on the weighted mean BEFORE the filter (csrc/mppi_variance.hpp)
  temperature        tests/emul.py: the host builds of csrc/host_search.hpp
  the draw           noise_ref.ideal_normals at the GLOBAL sample index, then the AR(1) statement of
                     test_colored_noise_host.py along the horizon, then the per-step sigma — the sampler's order

tick(pb, carry, eps32) restates one tick; `dtype` switches the tail between float64 and its float32 rounding; `wrong` names a
deliberate misreading (WRONG) that test_solve_ref_host.py uses to prove that a case can tell right from wrong; `given`
splices in a device's own U and costs, as the single-feature GPU tests do, so that the |c| / lambda amplification of a last
cost bit stays out of the comparison of the tail.
"""
import itertools
import math

import numpy as np

import action_cost_ref as acref
import discs_ref as D
import emul
import mlp_ref as ML
import noise_ref as nr
import particle_cases as pc
import racing_discs_ref as RD
import soft_discs_ref as SD
from helpers import MODEL_CFG, nav2d_env_fixture, oracle_problem, orc, racing_env_fixture
from pi_mpc import _host
from stats_cases import softplus32
from test_colored_noise_host import alpha_of
from test_colored_noise_host import restate as ar1_32
from test_covariance_host import numpy_step as cov_step32
from test_gpu_covariance import restate as cov_restate64
from test_gpu_covariance import weights64

f32, f64 = np.float32, np.float64
SEED = 42  # MPPI's default seed: what every rig of the GPU suite draws with

WRONG = ("g_base_sigma", "scale_then_filter", "var_on_filtered", "explore_inherits_in_var", "local_inherit",
         "search_on_particle0", "worst_as_mean")


# ---------------------------------------------------------------------------------------------- models
class Model:
    """A rollout reference behind one interface: rollout(x0, U, dtype, states) -> dict(costs, boundary, scale, S, band) and
    single(x0, action) -> [T + 1, ds].  `boundary`: the samples the model's own test leaves out of a cost comparison (float64
    margin below 1e-3 cell / 1e-4 m: check_costs, soft_discs_ref._boundaries); `band`: a per-sample limit where the model's
    test has one of its own (mlp_ref.band), else None and `limit` (of the cost scale) holds."""
    limit = 2e-6       # COST_TOL of test_gpu_parity.py, PARITY of discs_ref.py, the 2e-6 of test_gpu_soft_discs.py
    own_states = False  # the float64 costs are judged on the device's own states (soft_discs_ref says why)

    def single(self, x0, action):
        return self.rollout(x0, np.asarray(action, f32)[None], f64)["S"][0]


class OracleModel(Model):
    def __init__(self, name, ref_path=None):
        self.name, self.ref_path = name, ref_path
        self.ds, self.dc = orc.MODEL_DIMS[orc.MODEL_IDS[name]]
        cfg = MODEL_CFG[name]
        self.u_min, self.u_max, self.sigmas = f32(cfg["u_min"]), f32(cfg["u_max"]), f32(cfg["sigmas"])

    def rollout(self, x0, U, dtype=f64, states=None):
        U = np.ascontiguousarray(U, f32)
        N, T, _ = U.shape
        P = oracle_problem(self.name, N, T, ref_path=self.ref_path)
        # (U is clamped already and the clamp is idempotent: around a zero mean the oracle rolls out U itself)
        r = P.rollout_cost(x0, np.zeros((T, self.dc), f32), U, want_S=True, want_margin=True)
        c = r["costs"].astype(dtype)
        return dict(costs=c, boundary=~(r["margin"] > 1e-3), scale=float(np.abs(c).max()), S=r["S"], band=None)

    def single(self, x0, action):
        a = np.ascontiguousarray(action, f32)
        return oracle_problem(self.name, 1, a.shape[0], ref_path=self.ref_path).rollout_single(f32(x0), a)


class _DiscModel(Model):
    def _finish(self, r, dtype, keep_near=True):
        b = (r["near"] | r["edge"]) if keep_near else r["edge"]
        if dtype != f64:  # (the boundary rule is a float64 notion: the fp32 run carries none)
            b = np.zeros(len(r["costs"]), bool)
        return dict(costs=r["costs"], boundary=b, scale=r["scale"], S=r["S"], band=None)


class SoftNavModel(_DiscModel):
    """nav2d with soft moving discs (soft_discs_ref.rollout_nav2d)"""
    own_states = True

    def __init__(self, P, grid, table, reach, skirt):
        self.name, self.ds, self.dc = "nav2d_discs_soft", 3, 2
        self.P, self.grid, self.table, self.skirt = P, grid, np.ascontiguousarray(table, f32), float(skirt)
        self.ab = SD.coefficients(reach, skirt)
        self.u_min, self.u_max, self.sigmas = D.U_MIN, D.U_MAX, D.SIGMAS

    def rollout(self, x0, U, dtype=f64, states=None):
        r = SD.rollout_nav2d(self.P, self.grid, self.table, x0, U, self.ab[0], self.ab[1], dtype, states=states)
        return self._finish(r, dtype, keep_near=self.skirt != 1.0)  # (skirt = 1: continuous at the rim)


class RacingDiscModel(_DiscModel):
    """racing among moving discs (racing_discs_ref.rollout)"""

    def __init__(self, P, grids, ref, table):
        self.name, self.ds, self.dc = "racing_discs", 4, 2
        self.P, self.grids, self.ref, self.table = P, grids, np.ascontiguousarray(ref, f32), np.ascontiguousarray(table, f32)
        self.u_min, self.u_max, self.sigmas = RD.U_MIN, RD.U_MAX, RD.SIGMAS

    def rollout(self, x0, U, dtype=f64, states=None):
        return self._finish(RD.rollout(self.P, self.grids, self.ref, self.table, x0, U, dtype, states=states), dtype)


class MlpModel(Model):
    def __init__(self, cs):
        self.cs, self.name, self.ds, self.dc = cs, "mlp4%d" % cs["dc"], 4, cs["dc"]
        self.u_min, self.u_max, self.sigmas = f32(cs["u_min"]), f32(cs["u_max"]), f32(cs["sigmas"])

    def _run(self, x0, U, dtype):
        cs = self.cs
        return ML.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], x0, U, dtype)

    def rollout(self, x0, U, dtype=f64, states=None):
        c, S, mag = self._run(x0, U, dtype)
        band = None
        if dtype == f64:  # mlp_ref.band: 4 x the fp32 restatement's own distance from float64, floored
            band = ML.band(self._run(x0, U, f32)[0], c, mag)[0]
        return dict(costs=c, boundary=np.zeros(len(c), bool), scale=float(np.abs(c).max()), S=S, band=band)


_world = {}


def host_world(kind):
    """P and grids of the two map models from the committed fixtures (tests/test_soft_discs_host.world)"""
    if kind not in _world:
        if kind == "nav":
            e = nav2d_env_fixture()
            grid = (np.ascontiguousarray(e["map"], np.uint8), float(e["cell"]), float(e["origin"][0]), float(e["origin"][1]))
            _world[kind] = dict(P=f32(orc.nav2d_params()), grids=(grid,))
        else:
            e = racing_env_fixture()
            geom = (float(e["cell"]), float(e["origin"][0]), float(e["origin"][1]))
            _world[kind] = dict(P=f32(orc.racing_params()), start=f32(e["start_state"]), path=f32(e["center_path"]),
                                x_hi=float(e["x_lim"][1]),
                                grids=tuple((np.ascontiguousarray(e[k], np.uint8),) + geom for k in ("obst", "lane")))
    return _world[kind]


# ---------------------------------------------------------------------------------------------- the families and the features
FAMILIES = ("nav_soft", "racing_discs", "mlp42", "pendulum", "cartpole")
FEATURES = ("AC", "CN", "CV", "PR", "EX", "SG", "TL", "SH")
RULES = ("ESSPS", "LBPS_BRENT", "LBPS_GRID", "MPO")
SOFTNESS = (2.0, 1.0)          # reach > 1, skirt > 0
NAV_TABLE, RACING_TABLE = "n8", "n3"   # eight discs in every nav case
MLP_CASE = "mlp42_relu_2l_res"  # relu: bit for bit at math level 0
PARTICLES, CVAR_K = 3, 2
BETA = f32([0.9, 0.3])
EXPLORATION = 0.3
COV = dict(rate=0.5, floor=1e-4, smin_of_sigma=0.2, smax_of_sigma=3.0)
AC_WEIGHT = 1.0
# fixed temperatures per tick (mppi_solve takes one per solve): for every pair and tick the value of a four-per-decade ladder
# that brings the float64 ESS on the host normals closest to N / 5 (MPO pairs: the dual's start, for all three ticks; the
# searched pairs need none).  test_solve_ref_host.py::test_cases_are_well_posed holds every tick to ess_window(N).
_LAMBDAS = {
    ('AC', 'CN'): (100.0, 0.1, 0.0316),  # ESS / N [0.04, 0.18, 0.14]
    ('AC', 'CV'): (100.0, 10.0, 3.16),  # ESS / N [0.04, 0.2, 0.24]
    ('AC', 'PR'): (0.178, 0.1, 0.1),  # ESS / N [0.16, 0.23, 0.26]
    ('AC', 'EX'): (1.78, 1.0, 0.562),  # ESS / N [0.23, 0.16, 0.19]
    ('AC', 'SG'): (0.0562, 0.0316, 0.0316),  # ESS / N [0.07, 0.2, 0.2]
    ('AC', 'TL'): (178.0, 178.0, 178.0),  # ESS / N [0.09]
    ('AC', 'SH'): (100.0, 31.6, 5.62),  # ESS / N [0.23, 0.23, 0.24]
    ('CN', 'CV'): (0.1, 0.0562, 0.0562),  # ESS / N [0.2, 0.16, 0.27]
    ('CN', 'PR'): (1.78, 0.562, 0.01),  # ESS / N [0.28, 0.19, 0.21]
    ('CN', 'EX'): (0.0316, 0.1, 0.1),  # ESS / N [0.18, 0.23, 0.24]
    ('CN', 'SG'): (5.62, 10.0, 5.62),  # ESS / N [0.12, 0.24, 0.21]
    ('CN', 'TL'): None,
    ('CN', 'SH'): (56.2, 0.1, 0.01),  # ESS / N [0.23, 0.17, 0.23]
    ('CV', 'PR'): (0.0178, 0.0316, 0.0562),  # ESS / N [0.17, 0.17, 0.24]
    ('CV', 'EX'): (1.0, 1.0, 0.562),  # ESS / N [0.19, 0.26, 0.13]
    ('CV', 'SG'): (56.2, 10.0, 0.178),  # ESS / N [0.17, 0.19, 0.3]
    ('CV', 'TL'): None,
    ('CV', 'SH'): (0.1, 0.1, 0.0562),  # ESS / N [0.23, 0.34, 0.23]
    ('PR', 'EX'): (5.62, 5.62, 5.62),  # ESS / N [0.31, 0.12, 0.15]
    ('PR', 'SG'): (100.0, 17.8, 0.178),  # ESS / N [0.27, 0.24, 0.24]
    ('PR', 'TL'): None,
    ('PR', 'SH'): (1.0, 1.0, 0.562),  # ESS / N [0.16, 0.22, 0.16]
    ('EX', 'SG'): (0.1, 0.1, 0.1),  # ESS / N [0.23, 0.27, 0.3]
    ('EX', 'TL'): None,
    ('EX', 'SH'): (0.0178, 0.0316, 0.0178),  # ESS / N [0.21, 0.19, 0.19]
    ('SG', 'TL'): None,
    ('SG', 'SH'): (1.0, 1.0, 0.562),  # ESS / N [0.16, 0.21, 0.14]
    ('TL', 'SH'): (0.0178, 0.0178, 0.0178),  # ESS / N [0.18]
}
# device temperature rules: (target ESS as a share of N | delta, lambda_min, lambda_max)
RULE_ARGS = {"ESSPS": (0.15, 1e-3, 1e5), "LBPS_BRENT": (0.5, 1e-3, 1e3), "LBPS_GRID": (0.5, 1e-3, 1e3), "MPO": (0.0, 0.0, 0.0)}
MPO_EPS, MPO_LR = 0.1, 0.2

# (pair -> family, rule): the rotation.  test_solve_ref_host.py::test_rotation_covers holds it to the claim: every feature
# meets every family at least once, TL meets every rule at least once.
_ROTATION = {
    ("AC", "CN"): "nav_soft", ("AC", "CV"): "racing_discs", ("AC", "PR"): "mlp42", ("AC", "EX"): "pendulum",
    ("AC", "SG"): "cartpole", ("AC", "TL"): "nav_soft", ("AC", "SH"): "racing_discs",
    ("CN", "CV"): "mlp42", ("CN", "PR"): "pendulum", ("CN", "EX"): "cartpole", ("CN", "SG"): "racing_discs",
    ("CN", "TL"): "mlp42", ("CN", "SH"): "nav_soft",
    ("CV", "PR"): "cartpole", ("CV", "EX"): "pendulum", ("CV", "SG"): "nav_soft", ("CV", "TL"): "cartpole",
    ("CV", "SH"): "mlp42",
    ("PR", "EX"): "racing_discs", ("PR", "SG"): "nav_soft", ("PR", "TL"): "racing_discs", ("PR", "SH"): "pendulum",
    ("EX", "SG"): "mlp42", ("EX", "TL"): "nav_soft", ("EX", "SH"): "cartpole",
    ("SG", "TL"): "pendulum", ("SG", "SH"): "pendulum",
    ("TL", "SH"): "cartpole",
}
_RULE_OF = {("AC", "TL"): "MPO", ("CN", "TL"): "LBPS_BRENT", ("CV", "TL"): "LBPS_GRID", ("PR", "TL"): "ESSPS",
            ("EX", "TL"): "LBPS_GRID", ("SG", "TL"): "ESSPS", ("TL", "SH"): "MPO"}
_WORST_RISK = {("PR", "SG"), ("PR", "SH")}   # the cases whose measure is the worst case (the others: CVaR(2) of 3)
_WIDEST_SG = {("CN", "SG")}                  # the Savitzky-Golay window at the widest the horizon admits
PAIRS = tuple(itertools.combinations(FEATURES, 2))
TICKS = 3


def widest_window(T):
    """tests/test_gpu_lds_boundaries.py::widest_window: odd, <= 255, window / 2 <= 2T - 1"""
    return min(255, 2 * (2 * T - 1) + 1)


def pair_id(pair):
    return "x".join(pair)


class Shape:
    """family, N, T, dims and inherit_count of a pair: what a handle is created with, before any model exists"""

    def __init__(self, pair, family=None):
        self.pair = tuple(pair)
        self.family = _ROTATION[self.pair] if family is None else family   # (another family: the solver-level cases)
        self.dc = 1 if self.family in ("pendulum", "cartpole") else 2
        self.T = 5 if self.dc == 2 else 7                     # dc = 2: a row of 10 floats, three float4 groups, the last partial
        self.N = 320 if "SH" in self.pair else 200            # five tiles: a full block and one more | a partial last tile
        self.inherit = int(self.N * (1 - EXPLORATION)) if "EX" in self.pair else self.N


def shape_of(pair):
    return Shape(pair)


class Problem:
    """What one case fixes: the model, the shapes, which features are on and with what."""

    def __init__(self, pair, model, x0, features=None, family=None):
        self.pair = tuple(pair)
        self.family = _ROTATION[self.pair] if family is None else family
        self.model, self.x0 = model, f32(x0)
        self.on = set(self.pair if features is None else features)
        self.dc, self.ds = model.dc, model.ds
        shape = Shape(self.pair, family)                      # (the shapes belong to the pair, not to what a variant drops)
        assert shape.dc == self.dc
        self.T, self.N = shape.T, shape.N
        self.offset, self.n = 0, self.N                       # the window of the global samples this handle owns
        self.u_min, self.u_max, self.sigmas = f32(model.u_min), f32(model.u_max), f32(model.sigmas)
        self.lams = _LAMBDAS[self.pair] or (1.0, 1.0, 1.0)
        self.rule = _RULE_OF.get(self.pair) if "TL" in self.on else None
        self.risk = ("worst", 1) if self.pair in _WORST_RISK else ("cvar", CVAR_K)
        self.beta = BETA[:self.dc] if "CN" in self.on else None
        self.cov = dict(rate=COV["rate"], floor=COV["floor"], smin=f32(COV["smin_of_sigma"] * self.sigmas),
                        smax=f32(COV["smax_of_sigma"] * self.sigmas)) if "CV" in self.on else None
        self.ac_weight = AC_WEIGHT if "AC" in self.on else None
        self.inherit = int(self.N * (1 - EXPLORATION)) if "EX" in self.on else self.N
        self.sg = None
        if "SG" in self.on:
            w = widest_window(self.T) if self.pair in _WIDEST_SG else 5
            self.sg = _host.savitzky_golay_coeffs(w, 3)

    def without(self, feature):
        return Problem(self.pair, self.model, self.x0, self.on - {feature})

    def window(self, offset, n):
        """The same problem seen by a handle that owns the samples [offset, offset + n) of the global N"""
        q = Problem(self.pair, self.model, self.x0, self.on)
        q.offset, q.n = int(offset), int(n)
        return q

    def particles(self, x):
        """[P, ds] around the nominal state (the first IS the nominal state), or None"""
        if "PR" not in self.on:
            return None
        v = np.random.default_rng(7).normal(0.0, 0.05, self.ds)   # (one on either side: neither the nominal state nor one
        return (f32(x)[None] + np.stack([0.0 * v, v, -v])).astype(f32)  # particle is the worst for every sample)

    def mean0(self):
        """A warm start off zero (the term, the exploration split and the variance's centre all need one), inside the bounds"""
        t = np.arange(self.T, dtype=f64)[:, None]
        k = np.arange(self.dc, dtype=f64)[None]
        mid, half = 0.5 * (self.u_max + self.u_min).astype(f64), 0.5 * (self.u_max - self.u_min).astype(f64)
        return (mid + 0.35 * half * np.cos(0.9 * t + 1.3 * k + 0.4)).astype(f32)

    def rule_args(self):
        p, lo, hi = RULE_ARGS[self.rule]
        return (p * self.N if self.rule == "ESSPS" else p), lo, hi

    def carry0(self):
        tl = None
        if self.rule == "MPO":
            # {log T, m, v, t} and the temperature in force after mppi_mpo_reset(lams[0], ...): lams[0] itself, as fp32
            tl = dict(mpo=np.array([float(f32(math.log(self.lams[0]))), 0.0, 0.0, 0.0]), lam=float(f32(self.lams[0])))
        elif self.rule is not None:
            tl = dict(prev=0.0)
        return dict(t=0, x=self.x0.copy(), mean=self.mean0(), sigma=np.tile(self.sigmas, (self.T, 1)).astype(f32),
                    hist=np.zeros((self.T - 1, self.dc), f32) if self.sg is not None else None, tl=tl)


def host_model(family):
    """The family's model from committed fixtures alone (the GPU test builds the same class from its rig's own world)"""
    if family == "nav_soft":
        w = host_world("nav")
        table, x0 = D.case(NAV_TABLE, 5)
        return SoftNavModel(w["P"], w["grids"][0], table, *SOFTNESS), x0
    if family == "racing_discs":
        w = host_world("racing")
        table, x0 = RD.case(RACING_TABLE, 5, w["start"], w["x_hi"])
        return RacingDiscModel(w["P"], w["grids"], RD.window(w["path"], w["start"], 5), table), x0
    if family == "mlp42":
        return MlpModel(ML.case(MLP_CASE)), ML.X0
    return OracleModel(family), f32({"pendulum": [3.0, 0.1], "cartpole": [0.01, 0.0, 0.02, 0.0]}[family])


def host_problem(pair):
    model, x0 = host_model(_ROTATION[tuple(pair)])
    return Problem(pair, model, x0)


# ---------------------------------------------------------------------------------------------- the draw
def ar1(xi, beta, dtype=f64):
    """z[N, T, dc] from standard normals xi along the horizon, per control: the fp32 statement of test_colored_noise_host.py,
    or the same recurrence in float64 with the SAME fp32 beta and alpha (the library's coefficients)"""
    xi = np.asarray(xi, dtype)
    z = np.empty_like(xi)
    for k in range(xi.shape[2]):
        b = f32(beta[k])
        if b == 0:
            z[:, :, k] = xi[:, :, k]
        elif dtype == f32:
            z[:, :, k] = ar1_32(xi[:, :, k], b)
        else:
            a, bb = float(alpha_of(b)), float(b)
            z[:, 0, k] = xi[:, 0, k]
            for t in range(1, xi.shape[1]):
                z[:, t, k] = bb * z[:, t - 1, k] + a * xi[:, t, k]
    return z


def philox_normals(solve_idx, first, n, cols, seed=SEED):
    """float64 [n, cols]: the device stream's standard normals of the GLOBAL samples first .. first + n - 1 (noise_ref)"""
    return nr.ideal_normals(seed, solve_idx, first, n, -(-cols // 4))[:, :cols]


def numpy_normals(solve_idx, first, n, cols):
    """The same interface on numpy's generator (the CPU tests): a function of the solve index and the GLOBAL sample index"""
    return np.random.default_rng([97, int(solve_idx)]).standard_normal((first + n, cols))[first:]


def draw(solve_idx, first, n, T, dc, beta, sigma_table, dtype=f64, wrong=(), normals=philox_normals):
    """eps[n, T, dc] of the samples first .. first + n - 1 (GLOBAL indices): the normals, the filter, the per-step sigma"""
    xi = normals(solve_idx, first, n, T * dc).reshape(n, T, dc).astype(dtype)
    s = np.broadcast_to(np.asarray(sigma_table, f32), (T, dc)).astype(dtype)[None]
    beta = np.zeros(dc, f32) if beta is None else beta
    if "scale_then_filter" in wrong:
        return ar1((xi * s).astype(dtype), beta, dtype)
    return (ar1(xi, beta, dtype) * s).astype(dtype)


def draw_bound(beta, sigma_table, T, dc, pointwise):
    """|device eps - float64 eps| allowed per element, from `pointwise` = the limit test_gpu_noise_domain.py holds one standard
    normal to: the recurrence passes an error on as beta * previous + alpha * this, each of its three fp32 operations adds
    2^-24 of its result (|z| <= Z, Z = the largest radius times (beta + alpha)), the product with sigma one more."""
    beta = np.zeros(dc, f32) if beta is None else beta
    s = np.broadcast_to(np.asarray(sigma_table, f64), (T, dc))
    out = np.empty((T, dc))
    for k in range(dc):
        b, a = float(beta[k]), float(alpha_of(beta[k])) if beta[k] else 1.0
        Z = 5.7682 * (b + a)
        e = pointwise
        for t in range(T):
            if t and b:
                e = b * e + a * pointwise + 3.0 * 2.0 ** -24 * Z
            out[t, k] = (e + 2.0 ** -24 * Z) * s[t, k]
    return out


# ---------------------------------------------------------------------------------------------- the tick
def inherits(pb, local=False):
    i = np.arange(pb.n, dtype=np.int64) + (0 if local else pb.offset)
    return i < pb.inherit


def actions(pb, mean, eps32, local=False, everyone=False):
    """U = clamp(mean_i + eps), fp32: mean_i = 0 for the samples whose GLOBAL index is >= inherit_count.  One exactly rounded
    sum and a clamp: the value every reference of the suite takes as its input, whatever precision it then works in."""
    inh = np.ones(pb.n, bool) if everyone else inherits(pb, local)
    m = np.where(inh[:, None, None], np.asarray(mean, f32)[None], f32(0.0)).astype(f32)
    return np.clip((m + np.asarray(eps32, f32)).astype(f32), pb.u_min, pb.u_max).astype(f32)


def stats5(costs32, lam):
    """{cmin, cmax, sum e, sum e^2, sum e*c} as mppi_softmax_stats defines them (tests/host_emul/search.cpp::stats_of): the
    weights of weights64"""
    c = np.asarray(costs32, f32)
    e, _ = weights64(c, lam)
    return np.array([float(c.min()), float(c.max()), e.sum(), (e * e).sum(), (e * c.astype(f64)).sum()])


def temperature(pb, tl, costs32, t=0):
    """-> (the temperature this tick's weights use, the temperature the term saw when the rollout started, next `tl`)"""
    if pb.rule is None:
        return pb.lams[t], pb.lams[t], None
    c = np.ascontiguousarray(costs32, f32)
    p, lo, hi = pb.rule_args()
    if pb.rule == "MPO":  # the dual's current temperature weighs; it steps afterwards on this tick's costs
        st = np.array(tl["mpo"], f64)
        lam = float(tl["lam"])
        new, lam_next = emul.mpo_step_stats(st, MPO_EPS, MPO_LR, stats5(c, softplus32(st[0])))
        return lam, lam, dict(mpo=new, lam=lam_next)
    if pb.rule == "ESSPS":
        lam = emul.essps(c, p, lo, hi, lam_prev=tl["prev"], grid_argument=True)
    elif pb.rule == "LBPS_BRENT":
        lam = emul.lbps(c, p, lo, hi)[0]
    else:
        lam = emul.lbps_grid(c, p, lo, hi)
    return lam, tl["prev"], dict(prev=lam)   # (the term: the previous tick's temperature, 0 on the first)


def term_lambda(pb, tl, t=0):
    """The temperature the control-cost term is scaled with: it is read when the rollout STARTS"""
    if pb.rule is None:
        return pb.lams[t]
    if pb.rule == "MPO":
        return float(tl["lam"])
    return tl["prev"]


def fold(matrix, mode, k, dtype):
    if dtype == f32:
        return _host.fold_particle_costs(matrix, mode, k)
    return pc.fold64(matrix, mode, k)


def tick(pb, carry, eps32, dtype=f64, wrong=(), given=None, states=None):
    """One tick of `pb` from `carry` = dict(t, x, mean, sigma, hist, tl) on the noise eps32[n, T, dc] of this handle's samples.
    given: dict(U=, costs=, lambda=) of a device, used from where they arise on (the reference's own are still returned).
    states: a device's own state sequences [n, T + 1, ds] (one per particle while particles are set) for the models whose
    float64 costs are judged on them (Model.own_states)."""
    given = given or {}
    model, T, dc = pb.model, pb.T, pb.dc
    x, mean = f32(carry["x"]), f32(carry["mean"])
    out = {}
    out["U_ref"] = actions(pb, mean, eps32, local="local_inherit" in wrong)
    U32 = np.asarray(given["U"], f32) if "U" in given else out["U_ref"]
    out["U"], U = U32, U32.astype(dtype)
    # ---- costs: per particle, folded, the term behind the fold
    parts = pb.particles(x)
    out["particles"] = parts
    if parts is None:
        r = model.rollout(x, U, dtype, states=states)
        base, out["matrix"] = r["costs"], None
        boundary, band = r["boundary"], r["band"]
    else:
        rows = [model.rollout(p, U, dtype, states=None if states is None else states[m]) for m, p in enumerate(parts)]
        out["matrix"] = np.stack([q["costs"] for q in rows])
        mode, k = ("mean", 1) if "worst_as_mean" in wrong else pb.risk
        base = fold(out["matrix"].astype(f32) if dtype == f32 else out["matrix"], mode, k, dtype)
        boundary = np.any([q["boundary"] for q in rows], axis=0)
        band = None if rows[0]["band"] is None else np.max([q["band"] for q in rows], axis=0)
    out["folded"], out["boundary"], out["band"] = base, boundary, band
    costs = base
    lam_term = term_lambda(pb, carry["tl"], carry["t"])
    if pb.ac_weight is not None:
        g = acref.g32(mean, pb.sigmas if "g_base_sigma" in wrong else f32(carry["sigma"]))
        kappa = acref.kappa32(pb.ac_weight, lam_term)
        out["g"], out["kappa"] = g, kappa
        if dtype == f32:
            costs = acref.total32(base, kappa, acref.A32(g, U.astype(f32)))
        else:
            costs = base + float(kappa) * acref.A64(g, U.astype(f32))[0]
    out["costs"] = costs
    out["scale"] = float(np.abs(np.asarray(costs, f64)).max())
    c32 = np.asarray(given["costs"], f32) if "costs" in given else np.asarray(costs).astype(f32)
    out["costs32"] = c32
    # ---- the temperature, the weights, the summary
    search_on = c32
    if "search_on_particle0" in wrong and out["matrix"] is not None:
        search_on = out["matrix"][0].astype(f32)
    lam, _, tl_next = temperature(pb, carry["tl"], search_on, carry["t"])
    out["lambda_ref"] = lam
    if "lambda" in given:  # (the tail of a device's tick is judged at the device's own temperature, once that has been compared)
        lam = float(given["lambda"])
    out["lambda"], out["lambda_term"] = lam, lam_term
    e, ess = weights64(c32, lam)
    if dtype == f32:
        e = e.astype(f32)
        se, se2, sec = e.sum(dtype=f32), (e * e).sum(dtype=f32), (e * c32).sum(dtype=f32)
        ubar = ((e[:, None, None] * U).astype(f32).sum(0, dtype=f32) / se).astype(f32)
    else:
        se, se2, sec = e.sum(), (e * e).sum(), (e * c32.astype(f64)).sum()
        ubar = ((e / e.sum())[:, None, None] * U).sum(0)   # (test_gpu_covariance.restate's own expression)
    out["weights"], out["ess"] = e / se, ess
    out["stats"] = np.array([float(c32.min()), float(se), float(se2), float(sec)])
    out["abs_ec"] = float((np.asarray(e, f64) * np.abs(c32.astype(f64))).sum())
    out["mean_w"] = ubar
    # ---- the filter
    action, hist = ubar, carry["hist"]
    if pb.sg is not None:
        action = _host.sg_filter_sequence(carry["hist"], np.asarray(ubar), pb.sg)
        hist = np.concatenate([carry["hist"][1:], action[0][None, :]]).astype(f32)
    out["action"], out["hist"] = np.asarray(action), hist
    # ---- the sigma table: centred on the weighted mean BEFORE the filter; U of the variance is U of the solve
    sigma = f32(carry["sigma"])
    if pb.cov is not None:
        cv = pb.cov
        Uv = actions(pb, mean, eps32, everyone=True).astype(dtype) if "explore_inherits_in_var" in wrong else U
        if dtype == f64 and "var_on_filtered" not in wrong:
            s_new, var = cov_restate64(Uv, c32, lam, sigma, rate=cv["rate"], floor=cv["floor"], smin=cv["smin"], smax=cv["smax"])
        else:
            centre = np.asarray(action, dtype) if "var_on_filtered" in wrong else ubar
            w = (e / se)[:, None, None]
            var = (w * (Uv - centre) ** 2).sum(0, dtype=dtype)
            if dtype == f32:
                full = lambda v: np.broadcast_to(f32(v), (T, dc)).ravel()  # noqa: E731
                s_new = cov_step32((sigma * sigma).astype(f32).ravel(), var.astype(f32).ravel(), full(cv["rate"]),
                                   full(cv["floor"]), full(cv["smin"]), full(cv["smax"])).reshape(T, dc)
            else:
                s2 = (1.0 - cv["rate"]) * sigma.astype(f64) ** 2 + cv["rate"] * (var + cv["floor"])
                s_new = np.clip(np.sqrt(s2), cv["smin"], cv["smax"])
        out["var"] = var
        sigma = s_new
    out["sigma"] = np.asarray(sigma)
    # ---- the batch-1 rollout from the NOMINAL state, the best samples, the carry
    a32 = np.asarray(action).astype(f32)
    out["states"] = model.single(x, a32)
    order = np.argsort(c32, kind="stable")[:4]
    out["top_order"] = order
    out["top_states"] = model.rollout(x, U[order], dtype)["S"]
    out["top_weights"] = np.asarray(out["weights"], f64)[order]
    out["carry"] = dict(t=carry["t"] + 1, x=f32(out["states"][1]), mean=a32, sigma=np.asarray(sigma).astype(f32), hist=hist, tl=tl_next)
    return out


def eps_for(pb, carry, solve_idx, wrong=(), normals=philox_normals, offset=None):
    """The fp32 statement of the draw for this handle's window, from the sigma table in force"""
    first = pb.offset if offset is None else offset
    return draw(solve_idx, first, pb.n, pb.T, pb.dc, pb.beta, carry["sigma"], f32, wrong, normals)


def tick_sharded(pb, carry, solve_idx, dtype=f64, wrong=(), normals=philox_normals, shards=2, drop_offset=False):
    """One tick of `shards` windows of the global N and the combined tail: every window forms its own U and costs from its own
    draw (the window's offset decides the normals AND who inherits the mean), the tail runs once on all of them — what
    mppi_finalize(num_shards) computes from the windows' summaries.  drop_offset: every window believes it starts at 0."""
    n = pb.N // shards
    parts = []
    for r in range(shards):
        w = pb.window(0 if drop_offset else r * n, n)
        parts.append(tick(w, carry, eps_for(w, carry, solve_idx, wrong, normals), dtype, wrong))
    cat = lambda key: np.concatenate([p[key] for p in parts])  # noqa: E731
    eps = np.concatenate([eps_for(pb.window(r * n, n), carry, solve_idx, wrong, normals) for r in range(shards)])
    out = tick(pb, carry, eps, dtype, wrong, given=dict(U=cat("U"), costs=cat("costs")))
    out["shards"] = parts
    out["costs"], out["boundary"] = cat("costs"), cat("boundary")  # (the windows' own, for the cost comparisons)
    return out


def closed_loop(pb, dtype=f64, wrong=(), normals=philox_normals, ticks=TICKS, sharded=False, drop_offset=False):
    """`ticks` ticks from pb.carry0(); solve index t + 1 at tick t (index 0 is a solver's constructor draw)"""
    carry, outs = pb.carry0(), []
    for t in range(ticks):
        if sharded:
            o = tick_sharded(pb, carry, t + 1, dtype, wrong, normals, drop_offset=drop_offset)
        else:
            o = tick(pb, carry, eps_for(pb, carry, t + 1, wrong, normals), dtype, wrong)
        outs.append(o)
        carry = o["carry"]
    return outs


# ---------------------------------------------------------------------------------------------- distances and limits
TOL = 1e-5  # tests/test_gpu_parity.py (actions, states), tests/test_gpu_covariance.py (the sigma table)


def rel(a, b):
    """helpers.rel_err"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def cost_excess(got, ref):
    """max over the samples the boundary rule keeps of |got - ref| / limit, the limit being the model's own: band per sample
    (mlp_ref.band) or `limit` of the cost scale.  -> (excess, samples left out)"""
    keep = ~ref["boundary"]
    err = np.abs(np.asarray(got, f64) - np.asarray(ref["costs"], f64))
    lim = ref["band"] if ref["band"] is not None else np.full(len(err), ref["limit"] * ref["scale"])
    lim = np.maximum(lim, 1e-300)
    return (float(np.max(err[keep] / lim[keep])) if keep.any() else 0.0), int((~keep).sum())


def boundary_cap(N):
    return max(1, N // 100)


def distances(a, b, pb):
    """{quantity: distance / limit} between two evaluations of one tick, in the units and against the limits the GPU test
    uses for each quantity (`b` is the reference side)"""
    ref = dict(costs=b["costs"], boundary=b["boundary"] | a["boundary"], band=b["band"], limit=pb.model.limit, scale=b["scale"])
    d = dict(costs=cost_excess(a["costs"], ref)[0], action=rel(a["action"], b["action"]) / TOL,
             states=rel(a["states"], b["states"]) / TOL)
    d["sigma"] = float(np.max(np.abs(a["sigma"].astype(f64) - b["sigma"]) / np.maximum(np.abs(b["sigma"]), 1e-30))) / TOL
    if a["hist"] is not None and b["hist"] is not None:
        d["hist"] = rel(a["hist"], b["hist"]) / TOL
    # (an LBPS minimum is flat to fp32 noise: helpers.same_lbps_minimum takes two temperatures within 1e-3 for the same)
    lim = 1e-3 if (pb.rule or "").startswith("LBPS") else LAMBDA_TOL
    d["lambda"] = abs(a["lambda"] - b["lambda"]) / abs(b["lambda"]) / lim
    return d


LAMBDA_TOL = 5e-6  # stats_cases.WARM_TOL: the widest limit test_gpu_stats_geometry.py holds a device temperature to


# ---------------------------------------------------------------------------------------------- the rotation's claims
def rotation():
    return {p: (_ROTATION[p], _RULE_OF.get(p)) for p in PAIRS}


def ess_window(N):
    """Where the float64 ESS of every tick of every case must lie: enough samples carry weight for the weighted sums to be
    sums, and few enough for the weights to matter"""
    return 5.0, 0.8 * N
