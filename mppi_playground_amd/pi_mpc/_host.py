"""Host-side pieces of MPPI.forward() that the north star keeps on the CPU: automatic temperature
tuning (ESSPS / LBPS / MPO) and Savitzky-Golay smoothing.  numpy/scipy only, fp32 where the reference
computes in fp32.  Citations are relative to the reference repo.
"""
from __future__ import annotations

import math

import numpy as np
from scipy.optimize import brentq, minimize_scalar

F32 = np.float32


def softmax_weights(costs: np.ndarray, lam: float) -> np.ndarray:
    """torch.softmax(-costs / lambda_, dim=0) in fp32 (src/pi_mpc/mppi.py:355,376,543,564)."""
    x = (-costs) / F32(lam)
    e = np.exp(x - x.max())
    return e / e.sum(dtype=F32)


def compute_ess(weights: np.ndarray) -> float:
    """ESS = 1 / sum(w^2) (src/pi_mpc/mppi.py:526-532)."""
    return 1.0 / float(np.sum(weights * weights, dtype=F32))


def essps_lambda(costs: np.ndarray, target_ess: float, lam_min: float, lam_max: float) -> float:
    """Effective-sample-size policy search (src/pi_mpc/mppi.py:351-370,559-566)."""
    ess_at_min = compute_ess(softmax_weights(costs, lam_min))
    ess_at_max = compute_ess(softmax_weights(costs, lam_max))
    if target_ess <= ess_at_min:
        return lam_min
    if target_ess >= ess_at_max:
        return lam_max
    return brentq(lambda lam: compute_ess(softmax_weights(costs, lam)) - target_ess, lam_min, lam_max)


def lbps_objective(lam: float, costs: np.ndarray, delta: float) -> float:
    """Negative lower bound of the expected return (src/pi_mpc/mppi.py:534-557)."""
    w = softmax_weights(costs, lam)
    ess = compute_ess(w)
    expected_return = -float(np.sum(w * costs, dtype=F32))
    cost_range = float(costs.max() - costs.min())
    penalty = cost_range * math.sqrt((1 - delta) / delta) / math.sqrt(ess)
    return -(expected_return - penalty)


def lbps_lambda(costs: np.ndarray, delta: float, lam_min: float, lam_max: float) -> float:
    """Lower-bound policy search (src/pi_mpc/mppi.py:341-349)."""
    res = minimize_scalar(lambda lam: lbps_objective(lam, costs, delta), bounds=(lam_min, lam_max),
                          method="bounded")
    return float(res.x)


# ---- the same searches driven by device-side softmax statistics ---------------------------------------
# `stats(lam)` returns {cmin, cmax, se, se2, sec} with e_i = exp((-c_i)/lam - (-cmin)/lam) summed over all
# samples (mppi_softmax_stats, combined across shards): the O(N) work stays on the GPU, the scalar
# root-finding stays here.
def ess_from_stats(st) -> float:
    return st["se"] * st["se"] / st["se2"]


def essps_lambda_stats(stats, target_ess: float, lam_min: float, lam_max: float) -> float:
    """src/pi_mpc/mppi.py:351-370 with ESS(lambda) evaluated on the device."""
    if target_ess <= ess_from_stats(stats(lam_min)):
        return lam_min
    if target_ess >= ess_from_stats(stats(lam_max)):
        return lam_max
    return brentq(lambda lam: ess_from_stats(stats(lam)) - target_ess, lam_min, lam_max)


ESSPS_LOG_WARM_FACTOR = math.log(1.5)  # csrc/host_search.hpp: the same constants, the same steps
ESSPS_LOG_FINE_RATIO = math.log(1.05)
ESSPS_CLUSTER = 22
ESSPS_NPT = 6
ESSPS_AGREE = 1.0e-5


def essps_first_grid(lam_prev, lam_min: float, lam_max: float, points: int = 32):
    """First grid of a search and its logs (csrc/host_search.hpp::essps_first_point): geometric over [lam_min, lam_max], or —
    given the previous root well inside the range — ESSPS_CLUSTER points over [prev/1.5, prev*1.5] and the rest spread over
    what is left on either side in proportion to its log-length, the end points included."""
    lo, hi = float(lam_min), float(lam_max)
    lmin, lmax = math.log(lo), math.log(hi)
    lf = ESSPS_LOG_WARM_FACTOR
    lp = math.log(lam_prev) if lam_prev is not None and lam_prev > 0.0 else None
    warm = lp is not None and points >= ESSPS_CLUSTER + 2 and lp - lf > lmin + 1e-3 and lp + lf < lmax - 1e-3
    j = np.arange(points, dtype=np.float64)
    if not warm:
        lg = lmin + (lmax - lmin) * j / (points - 1.0)
    else:
        s = points - ESSPS_CLUSTER
        clo, chi = lp - lf, lp + lf
        nb = min(max(int(s * (clo - lmin) / ((clo - lmin) + (lmax - chi)) + 0.5), 1), s - 1)
        na = s - nb
        below = lmin + (clo - lmin) * j / nb
        cluster = clo + (chi - clo) * (j - nb) / (ESSPS_CLUSTER - 1)
        above = chi + (lmax - chi) * (j - (nb + ESSPS_CLUSTER - 1)) / na
        lg = np.where(j < nb, below, np.where(j < nb + ESSPS_CLUSTER, cluster, above))
    lg[0], lg[-1] = lmin, lmax
    grid = np.exp(lg)
    grid[0], grid[-1] = lo, hi
    return grid, lg


def _essps_poly(lgrid, ess, target_ess, j0, npt):
    """Lagrange form of log(lambda)(ESS) at ESS = target through grid points j0 .. j0+npt-1; None unless ESS increases."""
    xs, ys = lgrid[j0:j0 + npt], ess[j0:j0 + npt]
    if not np.all(np.diff(ys) > 0):
        return None
    x = 0.0
    for a in range(npt):
        num = den = 1.0
        for b in range(npt):
            if b != a:
                num *= target_ess - ys[b]
                den *= ys[a] - ys[b]
        x += num / den * xs[a]
    return float(x)


def _essps_interpolate(grid, lgrid, ess, target_ess, i, j0):
    x = _essps_poly(lgrid, ess, target_ess, j0, ESSPS_NPT)
    if x is not None and lgrid[i - 1] <= x <= lgrid[i]:
        return math.exp(x)
    lo, hi, e0, e1 = float(grid[i - 1]), float(grid[i]), float(ess[i - 1]), float(ess[i])
    if e1 == e0:
        return 0.5 * (lo + hi)
    return lo + (hi - lo) * (target_ess - e0) / (e1 - e0)


def essps_lambda_grid(stats_multi, target_ess: float, lam_min: float, lam_max: float, points: int = 32,
                      lam_prev=None) -> float:
    """The same root as essps_lambda_stats (ESS(lambda) = target, ESS increasing in lambda), bracketed on
    geometric grids: `stats_multi(lams)` evaluates ESS for up to 32 temperatures in ONE pass over the costs, so
    two round trips shrink the bracket from [lam_min, lam_max] to a ratio of (lam_max/lam_min)**(1/31**2)
    (1.007 for [0.01, 10]) and an inverse polynomial interpolation in (ESS, log lambda) through the six grid points
    around it lands within ~1e-7 relative of brentq's answer over the whole range — instead of ~18 sequential
    probes, each a device round trip.  With `lam_prev` (the previous solve's root) the first grid is clustered around
    it (essps_first_grid) and ONE round trip is enough whenever the root has not left the cluster and the
    interpolation has visibly converged there (~1e-6 relative).  Same steps as csrc/host_search.hpp::essps_lambda."""
    assert points >= 2 * ESSPS_NPT
    grid, lgrid = essps_first_grid(lam_prev, lam_min, lam_max, points)
    ess = np.asarray(stats_multi(grid), np.float64)
    if target_ess <= ess[0]:  # same end-point rules as the reference (mppi.py:361-364)
        return lam_min
    if target_ess >= ess[-1]:
        return lam_max

    def bracket(ess):
        above = np.nonzero(ess >= target_ess)[0]
        return max(int(above[0]) if len(above) else points - 1, 1)

    i = bracket(ess)
    h = ESSPS_NPT // 2
    if h <= i <= points - h and np.all(np.diff(lgrid[i - h:i + h]) <= ESSPS_LOG_FINE_RATIO):
        x6, x4 = _essps_poly(lgrid, ess, target_ess, i - h, ESSPS_NPT), _essps_poly(lgrid, ess, target_ess, i - 2, 4)
        if x6 is not None and x4 is not None and lgrid[i - 1] <= x6 <= lgrid[i] and abs(x6 - x4) <= ESSPS_AGREE:
            return math.exp(x6)  # the first grid was fine around the root and the interpolation has converged: one pass
    lo, hi, llo, lhi = float(grid[i - 1]), float(grid[i]), float(lgrid[i - 1]), float(lgrid[i])
    lgrid = llo + (lhi - llo) * np.arange(points) / (points - 1.0)
    lgrid[0], lgrid[-1] = llo, lhi
    grid = np.exp(lgrid)
    grid[0], grid[-1] = lo, hi
    ess = np.asarray(stats_multi(grid), np.float64)
    i = bracket(ess)
    return _essps_interpolate(grid, lgrid, ess, target_ess, i, min(max(i - ESSPS_NPT // 2, 0), points - ESSPS_NPT))


def lbps_lambda_stats(stats, delta: float, lam_min: float, lam_max: float) -> float:
    """src/pi_mpc/mppi.py:341-349,534-557 with the softmax sums evaluated on the device."""

    def objective(lam):
        st = stats(lam)
        expected_return = -st["sec"] / st["se"]
        penalty = (st["cmax"] - st["cmin"]) * math.sqrt((1 - delta) / delta) / math.sqrt(ess_from_stats(st))
        return -(expected_return - penalty)

    return float(minimize_scalar(objective, bounds=(lam_min, lam_max), method="bounded").x)


class MpoTemperature:
    """MPO E-step dual on the temperature (src/pi_mpc/mppi.py:191-200,387-398): one Adam(lr=0.2) step
    per solve on loss = softplus(logT) * (eps + logsumexp(-c / softplus(logT))), then
    lambda = exp(logT).  The gradient is written out instead of using autograd:
      dL/dT = eps + LSE + (sum_i w_i c_i) / T,   dT/dlogT = sigmoid(logT).
    The two large terms cancel (|LSE| ~ |c|/T against |dL/dT| ~ 1), so WHERE the reference rounds to fp32 decides
    the result: its autograd keeps LSE as an fp32 scalar and forms the weights of the backward pass as
    exp(x_i - fl32(LSE)) — they sum to exp(LSE - fl32(LSE)), not to 1.  Both roundings are reproduced here
    (`lse32`, `scale`); evaluating the same formula in float64 differs from the reference by 2-10 % of the gradient
    on nav2d costs (c ~ 770, T ~ 0.8), this statement by ~1e-4.
    """

    def __init__(self, lam0: float = 1.0, epsilon: float = 0.1, lr: float = 0.2):
        self.log_temperature = F32(math.log(lam0))
        self.epsilon = epsilon
        self.lr, self.b1, self.b2, self.eps = lr, 0.9, 0.999, 1e-8
        self.m = F32(0.0)
        self.v = F32(0.0)
        self.t = 0

    def temperature(self) -> float:
        """softplus(logT) as the fp32 scalar of the dual (not the lambda used for the weights)."""
        return float(F32(math.log1p(math.exp(float(self.log_temperature)))))

    def step(self, costs: np.ndarray) -> float:
        T = F32(self.temperature())
        c = costs.astype(F32)
        x = ((-c) / T).astype(np.float64)  # fp32 quotients, like the device statistics
        e = np.exp(x - x.max())
        return self.step_from_sums(float(c.min()), float(e.sum()), float((e * c).sum()))

    def step_from_stats(self, st) -> float:
        """`st` = softmax statistics at lambda = self.temperature()."""
        return self.step_from_sums(st["cmin"], st["se"], st["sec"])

    def step_from_sums(self, cmin: float, se: float, sec: float) -> float:
        """cmin, se = sum e_i, sec = sum e_i c_i with e_i = exp((-c_i)/T - (-cmin)/T), T = self.temperature()."""
        lt = float(self.log_temperature)
        T = F32(self.temperature())
        xmax32 = F32(-F32(cmin)) / T
        lse32 = F32(xmax32 + F32(math.log(F32(se))))           # torch.logsumexp keeps an fp32 scalar
        scale = math.exp(float(xmax32) - float(lse32))          # what the backward pass's fp32 weights sum to / se
        dL_dT = F32(F32(F32(self.epsilon) + lse32) + F32(scale * sec / float(T)))
        g = F32(float(dL_dT) * (1.0 / (1.0 + math.exp(-lt))))
        self.t += 1
        self.m = F32(self.b1 * float(self.m) + (1 - self.b1) * float(g))
        self.v = F32(self.b2 * float(self.v) + (1 - self.b2) * float(g) * float(g))
        bc1 = 1 - self.b1 ** self.t
        bc2 = 1 - self.b2 ** self.t
        denom = math.sqrt(float(self.v)) / math.sqrt(bc2) + self.eps
        self.log_temperature = F32(lt - (self.lr / bc1) * float(self.m) / denom)
        return float(np.exp(self.log_temperature))


def savitzky_golay_coeffs(window_size: int, poly_order: int) -> np.ndarray:
    """First row of pinv(vander(-h..h)) (src/pi_mpc/mppi.py:568-596)."""
    if window_size % 2 == 0 or window_size <= poly_order:
        raise ValueError("window_size must be odd and greater than poly_order.")
    half = (window_size - 1) // 2
    idx = np.arange(-half, half + 1, dtype=np.float64)
    A = np.vander(idx, N=poly_order + 1, increasing=True)
    return np.linalg.pinv(A)[0].astype(F32)


def apply_savitzky_golay(y: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
    """Symmetric-flip padding + valid cross-correlation (src/pi_mpc/mppi.py:598-620)."""
    pad = len(coeffs) // 2
    yp = np.concatenate([y[:pad][::-1], y, y[-pad:][::-1]]).astype(F32)
    n = len(y)
    out = np.zeros(n, F32)
    for j, cj in enumerate(coeffs):
        out += yp[j:j + n] * cj
    return out


def sg_filter_sequence(history: np.ndarray, action_seq: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
    """Step 7 of forward() (src/pi_mpc/mppi.py:423-443): filter [history(T-1); a(T)], keep the last T."""
    T = action_seq.shape[0]
    prolonged = np.concatenate([history, action_seq], axis=0).astype(F32)
    out = np.zeros_like(prolonged)
    for i in range(prolonged.shape[1]):
        out[:, i] = apply_savitzky_golay(prolonged[:, i], coeffs)
    return out[-T:]


def check_covariance_args(adapt_covariance, cov_rate, cov_floor, sigma_min, sigma_max, dim_control, shard_samples,
                          noise_source):
    """Validate the covariance-adaptation keyword arguments of MPPI (the sketch at src/pi_mpc/mppi.py:400-418) and return
    (cov_rate, cov_floor, sigma_min[dc], sigma_max[dc]) as floats / float32 arrays (defaults 0 and +inf).  ValueError for a
    rate outside [0, 1], a negative floor, sigma_min > sigma_max (or negative) in any dimension, and for the two
    combinations the adaptation does not support."""
    rate, floor = float(cov_rate), float(cov_floor)
    if not 0.0 <= rate <= 1.0:
        raise ValueError(f"cov_rate must lie in [0, 1], got {cov_rate}")
    if not (floor >= 0.0 and np.isfinite(floor)):
        raise ValueError(f"cov_floor must be >= 0, got {cov_floor}")

    def vec(v, default):
        if v is None:
            return np.full(dim_control, default, np.float32)
        a = np.asarray(v.detach().cpu() if hasattr(v, "detach") else v, dtype=np.float32).reshape(-1)
        if a.shape != (dim_control,):
            raise ValueError(f"sigma_min / sigma_max must have shape ({dim_control},)")
        return a

    smin, smax = vec(sigma_min, 0.0), vec(sigma_max, np.inf)
    if not (np.all(smin >= 0.0) and np.all(smin <= smax)):
        raise ValueError("need 0 <= sigma_min <= sigma_max in every control dimension")
    if adapt_covariance and shard_samples:
        raise ValueError("adapt_covariance=True is not available with shard_samples=True: the weighted variance would need "
                         "a second exchange between the shards")
    if adapt_covariance and noise_source == "torch_cpu":
        raise ValueError("adapt_covariance=True is not available with noise_source='torch_cpu': every draw would need the "
                         "sigma table on the host")
    return rate, floor, smin, smax


def check_action_cost_args(action_cost, action_cost_weight, sigmas, adapt_covariance=False, cov_floor=1e-6, sigma_min=None):
    """Validate the keyword arguments of the control-cost term of MPPI (src/pi_mpc/mppi.py:294-316,330-336) and return the
    weight as a float.  ValueError for a negative or non-finite weight and, with the term on, for any sigmas[k] <= 0
    (the term divides by sigma^2) and for adapt_covariance=True with cov_floor == 0 and no positive sigma_min in every
    dimension (the adapted table could reach 0 and its inverse overflow)."""
    w = float(action_cost_weight)
    if not (w >= 0.0 and np.isfinite(w)):
        raise ValueError(f"action_cost_weight must be finite and >= 0, got {action_cost_weight}")
    if not action_cost:
        return w
    s = np.asarray(sigmas.detach().cpu() if hasattr(sigmas, "detach") else sigmas, dtype=np.float32).reshape(-1)
    if not np.all(s > 0.0):
        raise ValueError("action_cost=True needs sigmas > 0 in every control dimension (the term divides by sigma^2)")
    if adapt_covariance and not float(cov_floor) > 0.0:
        smin = None if sigma_min is None else np.asarray(
            sigma_min.detach().cpu() if hasattr(sigma_min, "detach") else sigma_min, dtype=np.float32).reshape(-1)
        if smin is None or not np.all(smin > 0.0):
            raise ValueError("action_cost=True with adapt_covariance=True needs cov_floor > 0 or a positive sigma_min in every "
                             "control dimension: the adapted sigma table could reach 0")
    return w


def check_noise_beta_args(noise_beta, dim_control, noise_source="philox", action_cost=False):
    """Validate the `noise_beta` keyword argument of MPPI (the lag-1 correlation of the AR(1) filter on the sampling noise)
    and return it as a float32 array [dim_control]: a float stands for every control dimension.  ValueError for a wrong
    length, an entry outside [0, 1) and — with any entry non-zero — for the two combinations the filter does not support."""
    b = np.asarray(noise_beta.detach().cpu() if hasattr(noise_beta, "detach") else noise_beta, dtype=np.float32)
    if b.ndim == 0:
        b = np.full(dim_control, b, np.float32)
    b = np.ascontiguousarray(b.reshape(-1), np.float32)
    if b.shape != (dim_control,):
        raise ValueError(f"noise_beta must be a float or have shape ({dim_control},)")
    if not np.all((b >= 0.0) & (b < 1.0)):
        raise ValueError(f"noise_beta must lie in [0, 1) in every control dimension, got {noise_beta}")
    if b.any() and noise_source == "torch_cpu":
        raise ValueError("noise_beta > 0 is not available with noise_source='torch_cpu': the filter would need a second "
                         "implementation on the host")
    if b.any() and action_cost:
        raise ValueError("noise_beta > 0 is not available with action_cost=True: the term's inverse covariance is diagonal in "
                         "time and would no longer be the KL term of the distribution sampled from")
    return b


# ---- risk-aware solves (include/mppi_hip.h: mppi_set_particles)
MAX_PARTICLES = 16                                # MPPI_MAX_PARTICLES
RISK_MODES = {"mean": 0, "worst": 1, "cvar": 2}  # MPPI_RISK_*


def check_risk_args(risk, risk_alpha):
    """Validate the `risk` / `risk_alpha` keyword arguments of MPPI and return (risk, risk_alpha as a float).  ValueError for
    an unknown measure and for risk_alpha outside (0, 1]."""
    if risk not in RISK_MODES:
        raise ValueError(f"risk must be 'mean', 'worst' or 'cvar', got {risk!r}")
    a = float(risk_alpha)
    if not (0.0 < a <= 1.0):
        raise ValueError(f"risk_alpha must lie in (0, 1], got {risk_alpha}")
    return risk, a


def risk_k(risk_alpha, P):
    """The number of worst particles CVaR averages: k = min(P, max(1, ceil(risk_alpha * P))), in float64."""
    return int(min(int(P), max(1, math.ceil(float(risk_alpha) * int(P)))))


def check_particles_shape(shape, dim_state):
    """Validate the shape of a particle table [P, dim_state] (set_state_particles); returns P.  ValueError for a wrong shape,
    P = 0 or P > 16."""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 2 or shape[1] != int(dim_state):
        raise ValueError(f"state particles: expected [P, {dim_state}], got {list(shape)}")
    if not 1 <= shape[0] <= MAX_PARTICLES:
        raise ValueError(f"state particles: P = {shape[0]}, need 1 <= P <= {MAX_PARTICLES} (None switches the feature off)")
    return shape[0]


def fold_particle_costs(matrix, mode, k=1):
    """The fold of include/mppi_hip.h (particle_fold_kernel) restated in numpy, in the header's operation order: matrix [P, N]
    fp32 -> [N] fp32.  `mode`: "mean" | "worst" | "cvar" (or MPPI_RISK_* 0 | 1 | 2); `k`: the worst particles averaged under
    CVaR, 1 <= k <= P.  Every operation rounds on its own in fp32, the division is the IEEE quotient.  A NaN among the P costs
    of a sample makes its folded cost NaN in every mode, as on the device."""
    c = np.ascontiguousarray(matrix, dtype=F32)
    if c.ndim != 2 or c.shape[0] < 1:
        raise ValueError(f"particle costs: expected [P, N], got {list(c.shape)}")
    P = c.shape[0]
    mode = RISK_MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError(f"unknown risk measure {mode!r}")
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 1:
            a = c[0].copy()
            for m in range(1, P):
                a = np.maximum(a, c[m])
        elif mode == 2:
            k = int(k)
            if not 1 <= k <= P:
                raise ValueError(f"CVaR needs 1 <= k <= P, got k = {k}, P = {P}")
            s = -np.sort(-c, axis=0)  # largest first (negation is exact; ties are interchangeable)
            a = s[0].copy()
            for j in range(1, k):
                a = (a + s[j]).astype(F32)
            a = (a / F32(k)).astype(F32)
        else:
            a = c[0].copy()
            for m in range(1, P):
                a = (a + c[m]).astype(F32)
            a = (a / F32(P)).astype(F32)
    a[np.isnan(c).any(axis=0)] = np.nan
    return a.astype(F32)
