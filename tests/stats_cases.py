"""Cases for the softmax statistics every automatic temperature rule stands on (mppi_search.hpp, capi_search.hip):
stats_partial_kernel + stats_combine_kernel (one temperature, 256-thread blocks) and stats_multi_block + stats_combine_columns
(32 temperatures, 1024-thread blocks).  The launch geometry restated from the headers' constants, the tables of sample counts,
where a single cost is placed, the cost vectors, the temperature sets, the float64 references over the argument each kernel
forms in fp32, and the limits.

Nothing here touches the GPU or the library.  tests/test_stats_cases_host.py asserts that the tables reach what they claim;
tests/test_gpu_stats_geometry.py runs them.
"""
from __future__ import annotations

import math
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mppi_playground_amd", "csrc")


# ------------------------------------------------------------------------------ the kernels' constants
def header_constants():
    """`constexpr int NAME = value;` lines of the headers the geometry depends on."""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("mppi_common.hpp", "mppi_search.hpp", "host_search.hpp"))
    out = {}
    for name in ("WAVE", "BLOCK", "STATS_BLOCKS", "STATS_THREADS", "STATS_L", "STATS_COMB_GROUPS", "BRENT_STAGE_MAX",
                 "LBPS_GRID_ROUNDS"):
        m = re.findall(r"^constexpr int %s = (\d+);" % name, text, re.M)
        assert len(m) == 1, name
        out[name] = int(m[0])
    return out


_K = header_constants()
WAVE, BLOCK = _K["WAVE"], _K["BLOCK"]
STATS_BLOCKS, STATS_THREADS, STATS_L = _K["STATS_BLOCKS"], _K["STATS_THREADS"], _K["STATS_L"]
STATS_COMB_GROUPS, BRENT_STAGE_MAX, LBPS_GRID_ROUNDS = _K["STATS_COMB_GROUPS"], _K["BRENT_STAGE_MAX"], _K["LBPS_GRID_ROUNDS"]
BRENT_LANES = WAVE          # blocks of lbps_brent_kernel's launch, at most
CHUNK = 32                  # costs a thread of stats_multi_block walks per round (a half-wave shares them)
BRENT_LDS_FIXED = 268 + 256  # sizeof(BrentLds) + the slack mppi_lbps_brent_device leaves


def _cdiv(a, b):
    return -(-int(a) // int(b))


def _clamp(v, lo, hi):
    return max(lo, min(hi, v))


def one_geometry(N):
    """(nvb, chain): blocks of stats_partial_kernel's grid (the Brent search's virtual blocks) and costs per thread."""
    nvb = _clamp(_cdiv(N, BLOCK), 1, STATS_BLOCKS)
    return nvb, _cdiv(N, nvb * BLOCK)


def multi_geometry(N):
    """(B, rounds) of stats_multi_kernel / essps_round_kernel: blocks of 1024 threads and rounds of their loop."""
    B = _clamp(_cdiv(N, STATS_THREADS), 1, STATS_BLOCKS)
    return B, _cdiv(N, B * STATS_THREADS)


def brent_geometry(N, lds_max=160 * 1024):
    """(grid, groups, staged) of lbps_brent_kernel: its blocks, the virtual blocks each of them runs, and whether the costs are
    staged in LDS (at most BRENT_STAGE_MAX per thread, and the copy has to fit the device's limit per block)."""
    nvb, per = one_geometry(N)
    groups = _cdiv(nvb, BRENT_LANES)
    staged = per <= BRENT_STAGE_MAX and 4 * per * BLOCK * groups + BRENT_LDS_FIXED <= lds_max
    return min(nvb, BRENT_LANES), groups, staged


def brent_staging_pair(lds_max=160 * 1024):
    """(N, N + 1) with STATS_BLOCKS virtual blocks on both sides of the staging limit of a device with `lds_max` bytes per block."""
    per = min(BRENT_STAGE_MAX, (lds_max - BRENT_LDS_FIXED) // (4 * BLOCK * _cdiv(STATS_BLOCKS, BRENT_LANES)))
    n = per * STATS_BLOCKS * BLOCK
    return n, n + 1


def last_chunk(N):
    """(live, chunk): live costs of the last chunk stats_multi_block sees with a live cost in it, and that chunk's index in its
    block (even: lanes 0 .. 31 of a wave, odd: lanes 32 .. 63)."""
    r = (N - 1) % STATS_THREADS + 1
    return (r - 1) % CHUNK + 1, (r - 1) // CHUNK


def block0_alone_in_last_round(N):
    B, rounds = multi_geometry(N)
    return rounds > 1 and N - (rounds - 1) * B * STATS_THREADS <= STATS_THREADS


# ------------------------------------------------------------------------------ the tables
# 32 temperatures.  (38 * 1024 + 5 is B = 39: 39 * 1024 + 5 already rounds up to 40 blocks.)
MULTI_SIZES = [1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2079, 38 * 1024 + 5, 39 * 1024 + 5, 40 * 1024, 40 * 1024 + 1,
               255 * 1024 + 1, 262144, 262145, 262144 + 100 * 1024 + 17, 524289, 787209]
# one temperature.  (32 768 and 49 152 are nvb = 128 and 192: the last virtual blocks of Brent groups 2 and 3.)
ONE_SIZES = [1, 63, 64, 65, 255, 256, 257, 16384, 16385, 32768, 32769, 49152, 49153, 65536, 65537, 65791, 131073, 2097152,
             2097153]
ALL_SIZES = sorted(set(MULTI_SIZES) | set(ONE_SIZES))
SEARCH_SIZES = [33, 1000, 1025, 40 * 1024 + 1, 262145, 600001]   # the ESSPS chain and the LBPS grid search
MPO_SIZES = [33, 1025, 65537, 262145]


def positions(N):
    """Indices at which a single cost is placed: both ends, the first index of the last block of either kernel, the edges of
    half-waves, waves and blocks, and both sides of the end of the first round of either grid.  Below N, ascending."""
    B, _ = multi_geometry(N)
    nvb, _ = one_geometry(N)
    want = [0, N - 1, (N - 1) // STATS_THREADS * STATS_THREADS, (N - 1) // BLOCK * BLOCK, 31, 32, 63, 64, 255, 256, 1023, 1024,
            B * STATS_THREADS - 1, B * STATS_THREADS, nvb * BLOCK - 1, nvb * BLOCK]
    return sorted({int(p) for p in want if 0 <= p < N})


# ------------------------------------------------------------------------------ cost vectors
LIVE, DEAD = 2.0, 2.0 + 1.0e6     # e = 1 and e = 0 exactly for every temperature up to 1e3
EQUAL = 3.25
PLATEAU, PEAK, PIT = 5.0, 7.0, 1.0


def one_live(N, at):
    c = np.full(N, DEAD, f32)
    c[np.asarray(at, np.int64)] = LIVE
    return c


def extreme_at(N, p, value):
    c = np.full(N, PLATEAU, f32)
    c[p] = value
    return c


def raised_max_at(N, p):
    """The smooth dense vector (pendulum-like) with its first cost raised to twice the maximum, and that cost swapped to p:
    the same costs in another order for every p, with a cost range that one element decides."""
    c = dense_costs(N, "brent2").copy()
    c[0] = 2.0 * c.max()
    c[0], c[p] = c[p], c[0]
    return c


def brent_cost_vector(rng, N, kind):
    """Cost vectors for the LBPS search: the shapes of the shipped models' costs and awkward ones."""
    if kind == 0:    # nav2d-like: distances + collision penalties
        c = rng.uniform(10, 40, N) + 1e4 * rng.integers(0, 30, N) * (rng.random(N) < 0.5)
    elif kind == 1:  # racing-like
        c = rng.uniform(300, 3000, N) + 1e4 * rng.integers(0, 25, N) * (rng.random(N) < 0.4)
    elif kind == 2:  # pendulum / cartpole-like: a smooth, narrow range
        c = rng.gamma(2.0, rng.uniform(0.5, 50.0), N) + rng.uniform(0, 100)
    elif kind == 3:  # a range of e^40
        c = np.exp(rng.uniform(-20, 20, N))
    elif kind == 4:  # mixed signs, any scale
        c = rng.standard_normal(N) * 10.0 ** rng.integers(-3, 6)
    elif kind == 5:  # all equal: the objective has no range term
        c = np.full(N, float(rng.uniform(-5, 5)))
    elif kind == 6:  # few distinct values
        c = rng.integers(0, max(2, N // 50), N).astype(np.float64)
    else:            # one clear winner
        c = rng.uniform(100, 200, N)
        c[int(rng.integers(0, N))] = 1.0
    return np.ascontiguousarray(c, dtype=np.float32)


BRENT_KINDS = 8


def essps_cost_shapes(rng, N):
    """name -> draw() of the ESSPS search's cost vectors: Gaussian, heavy-tailed, two clusters, a huge common offset, all equal
    (ESS = N at every temperature), one far outlier (ESS stays near 1).  The draws share `rng`, in the order they are called."""
    return {
        "gauss": lambda: rng.standard_normal(N) * 3.0 + 50.0,
        "gauss_small_spread": lambda: rng.standard_normal(N) * 0.02 + 7.0,
        "exponential": lambda: rng.exponential(5.0, N),
        "lognormal": lambda: np.exp(rng.standard_normal(N) * 1.5),
        "two_clusters": lambda: np.where(rng.random(N) < 0.05, rng.standard_normal(N) * 0.5, 40.0 + rng.standard_normal(N)),
        "offset_1e6": lambda: 1.0e6 + rng.standard_normal(N) * 4.0,
        "all_equal": lambda: np.full(N, 3.25),
        "one_outlier": lambda: np.concatenate([[-1.0e4], 100.0 + rng.standard_normal(N - 1)]),
    }


ESSPS_SHAPES = tuple(essps_cost_shapes(None, 1))
DENSE_KINDS = tuple(f"brent{k}" for k in range(BRENT_KINDS)) + ESSPS_SHAPES
# (N, kind) -> which draw of that kind is used, where draw 0 did not meet a limit with the float64 reference alone
# (tests/test_stats_cases_host.py); the limits themselves stay
REDRAW = {}


def dense_costs(N, kind):
    """The cost vector of (N, kind), fp32; the same array on every call."""
    i = DENSE_KINDS.index(kind)
    rng = np.random.default_rng([20, N, i, REDRAW.get((N, kind), 0)])
    if i < BRENT_KINDS:
        return brent_cost_vector(rng, N, i)
    return np.ascontiguousarray(essps_cost_shapes(rng, N)[kind](), f32)


# ------------------------------------------------------------------------------ temperatures
def _geometric(lo, hi, n=32):
    return np.exp(np.linspace(math.log(lo), math.log(hi), n)).astype(f32)


SET_NARROW = _geometric(0.01, 10.0)
SET_WIDE = _geometric(1.0e-3, 1.0e3)
SET_SHUFFLED = SET_WIDE[(13 * np.arange(32) + 5) % 32]       # all different, not monotone: a column in the wrong slot shows
TEMPERATURE_SETS = {"narrow": SET_NARROW, "wide": SET_WIDE, "count1": SET_NARROW[:1], "count31": SET_NARROW[:31],
                    "shuffled": SET_SHUFFLED}
# what the one-temperature kernel is run at: both ends and two inner values of either range
ONE_LAMBDAS = np.concatenate([SET_NARROW[[0, 10, 21, 31]], SET_WIDE[[0, 10, 21, 31]]])
EXACT_LAMBDAS = f32([1.0e-3, 1.0, 1.0e3])


# ------------------------------------------------------------------------------ float64 references
_pool = None


def pmap(fn, items):
    """map over a few threads (numpy and the host search library release the interpreter lock on large arrays)."""
    global _pool
    if _pool is None:
        _pool = ThreadPoolExecutor(max_workers=8)
    return list(_pool.map(fn, items))


def _sums(x32, c64, a64):
    e = np.exp(x32.astype(np.float64))
    return float(e.sum()), float(e @ e), float(e @ c64), float(e @ a64)


def reference_one(costs, lams):
    """[len(lams)][4] = {sum e, sum e^2, sum e*c, sum e*|c|} in float64 with stats_partial_thread's argument
    x = fl32(fl32(-c / lam) - fl32(-cmin / lam)) (numpy's float32 operations are IEEE) and e = exp(float64(x))."""
    c = np.asarray(costs, f32)
    cmin, nc = c.min(), -c
    c64 = c.astype(np.float64)
    a64 = np.abs(c64)
    return np.array(pmap(lambda lam: _sums(nc / f32(lam) - (-cmin) / f32(lam), c64, a64), list(lams)))


def reference_multi(costs, lams):
    """The same with stats_multi_block's argument x = fl32(fl32(cmin - c) * fl32(1 / lam))."""
    c = np.asarray(costs, f32)
    d = c.min() - c
    c64 = c.astype(np.float64)
    a64 = np.abs(c64)
    return np.array(pmap(lambda lam: _sums(d * (f32(1.0) / f32(lam)), c64, a64), list(lams)))


def underflow_floor(costs):
    """What fp32 cannot hold of sum e*c whatever the order of the sum: a weight below 2^-126 is a denormal, known to 2^-149
    absolute instead of 2^-24 relative, and so is a partial sum that small; 2^-149 * (sum |c| + N) bounds both.  It matters
    only where every cost of normal weight is 0 (integer costs with the minimum at 0 and exp(-1 / lambda) < 2^-126)."""
    c = np.abs(np.asarray(costs, np.float64))
    return 2.0 ** -149 * float(c.sum() + len(c))


def sums_error(got3, ref4, floor=0.0):
    """Largest of the errors of sum e and sum e^2 (relative to themselves) and of sum e*c (relative to sum e*|c|, beyond the
    `floor` of underflow_floor)."""
    got3, ref4 = np.asarray(got3, np.float64), np.asarray(ref4, np.float64)
    scale = np.stack([ref4[..., 0], ref4[..., 1], ref4[..., 3]], -1)
    diff = np.abs(got3 - ref4[..., :3])
    diff[..., 2] = np.maximum(0.0, diff[..., 2] - floor)
    # (sum e*|c| is 0 where every weighted cost is 0: then sum e*c has to be 0 too)
    err = np.where(scale > 0.0, diff / np.where(scale > 0.0, scale, 1.0), np.where(diff == 0.0, 0.0, np.inf))
    return float(np.max(err))


def ess64(costs, lam):
    c = np.asarray(costs, np.float64)
    e = np.exp(-(c - c.min()) / lam)
    return float(e.sum() ** 2 / (e @ e))


def essps_end_point(costs, target, lo, hi):
    """The end point the reference's rules return in float64 (mppi.py:361-364), or None where the root is inside."""
    if target <= ess64(costs, lo):
        return lo
    if target >= ess64(costs, hi):
        return hi
    return None


def essps_targets(N):
    return [N / 10, 0.9 * N, min(50.0, N / 2)]


def lbps_objective(cmin, cmax, se, se2, sec, delta):
    """host_search.hpp: lbps_objective, operation for operation (every one correctly rounded)."""
    expected_return = -sec / se
    penalty = (cmax - cmin) * math.sqrt((1.0 - delta) / delta) / math.sqrt(se * se / se2)
    return -(expected_return - penalty)


PLATEAU_KINDS = ("brent5", "brent6", "max_at_")   # equal costs, two cost values, 5.0 everywhere and 7.0 once


def on_one_plateau(costs, lam, lam_ref, delta):
    """The float64 LBPS objective at both temperatures and between them is one value (to 4 fp32 ulp): below some temperature
    every weight of such a vector is 0 or 1 and the objective constant, every point of that stretch is a minimiser, and which
    one a search returns is decided by its own rounding."""
    from helpers import lbps_objective64

    f = [lbps_objective64(costs, x, delta) for x in (lam, math.sqrt(lam * lam_ref), lam_ref)]
    return max(f) - min(f) <= 4 * float(np.finfo(f32).eps) * abs(f[0])


def grid_point(lo, hi, j, P=32):
    """host_search.hpp: essps_grid_point."""
    if j == 0:
        return lo
    if j == P - 1:
        return hi
    llo, lhi = math.log(lo), math.log(hi)
    return math.exp(llo + (lhi - llo) * float(j) / float(P - 1))


def softplus32(log_t):
    """MpoState::temperature(): softplus(log T) in double, rounded to fp32."""
    return f32(math.log1p(math.exp(float(f32(log_t)))))


def ulp32(a, b):
    """Distance of two fp32 values in units of the last place of the larger."""
    a, b = f32(a), f32(b)
    if a == b:
        return 0.0
    return abs(float(a) - float(b)) / float(np.spacing(max(abs(a), abs(b), np.finfo(f32).tiny)))


# ------------------------------------------------------------------------------ the limits
TOL = 1.0e-5
ESS_BAND = 1.0e-4          # |ESS64(lambda) - target| / target of a device search (test_device_softmax_stats_drive_the_same_temperature)
ESS_BAND_REFERENCE = 2.0e-5  # ... of the float64 search alone
COLD_TOL, WARM_TOL = 1.0e-12, 5.0e-6   # device chain against the host loop (test_essps_device_search_equals_the_host_loop_on_random_costs)
TWIN_TOL = 1.0e-12
MPO_ULP = 4
LBPS_DELTAS = (0.01, 0.1)
LAM_MIN, LAM_MAX = 0.01, 10.0


def chain_one(N):
    """Longest sequential fp32 chain of the one-temperature sums: a thread's costs, 6 butterfly steps, 3 folds."""
    return one_geometry(N)[1] + 6 + 3


def chain_multi(N):
    """... of the 32-temperature sums: 32 costs per round, the half-wave shuffle, 15 additions over the 16 waves."""
    return CHUNK * multi_geometry(N)[1] + 1 + 15


def limit(chain, tol=TOL):
    return max(tol, chain * 2.0 ** -24)
