"""Injected-summary cases for the tail of a solve (csrc/mppi_finalize.hpp: finalize_tail, reached through mppi_finalize): the
combine of the shard summaries, the normalisation, the Savitzky-Golay step with its warm start and history shift, and the
batch-1 rollout of the solution.  The constants the edges depend on restated from the sources' own lines, the three tables,
the inputs each case hands to the kernel and the float64 reference of the combine.

mppi_finalize(summaries_dev, num_shards, ...) takes summaries written by the caller; with the one shard {0, 1, 1, 0, A} the
tail's action is A bit for bit (f = exp(0) = 1, fma(1, A, 0) / 1), so a test can hand the tail any action sequence.

Nothing here touches the GPU or the library.  tests/test_tail_cases_host.py asserts that the tables reach what they claim;
tests/test_gpu_tail_geometry.py runs them.
"""
from __future__ import annotations

import os
import re
import zlib
from collections import namedtuple

import numpy as np

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mppi_playground_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mppi_hip.h")

TOL = 1e-5           # the project's plain limit (test_gpu_covariance.TOL); test_tail_cases_host.py says why no band is needed
DEAD_GAP = 1.0e4     # as reduce_cases.DEAD_GAP: fl32(x - (x + 1e4)) <= -1e4 and expf(-1e4) is exactly 0
DEAD_VALUE = 1.0e30  # what a dead shard's row and sums hold: large, finite, and gone after a factor of exactly 0


# ------------------------------------------------------------------------------ the sources' constants
# the admission rules of mppi_set_sg_filter (capi_solve.hip), as the source writes them
ADMISSION_LINES = (
    "if (!coeffs_host || window % 2 == 0 || window > 255) return fail(",
    "if (h->d.row > FIN_BLOCK) return fail(",
    "if (window / 2 > 2 * h->d.T - 1) return fail(",
    "const size_t hist_floats = (size_t)std::max(h->d.T - 1, 1) * h->dc;",
)


def source_constants():
    """FIN_BLOCK and the wave-rollout threshold of batch1_rollout from mppi_finalize.hpp, MPPI_SUMMARY_HEAD from the public
    header, the widest window from mppi_set_sg_filter."""
    fin = open(os.path.join(CSRC, "mppi_finalize.hpp")).read()
    solve = open(os.path.join(CSRC, "capi_solve.hip")).read()
    head = open(HEADER).read()
    out = {}
    for name, text, pattern in (("FIN_BLOCK", fin, r"^constexpr int FIN_BLOCK = (\d+);"),
                                ("WAVE_ROLLOUT_MAX_T", fin, r"^\s+if \(T <= (\d+)\) \{"),
                                ("MPPI_SUMMARY_HEAD", head, r"^#define MPPI_SUMMARY_HEAD (\d+)\b"),
                                ("SG_MAX_WINDOW", solve, r"window % 2 == 0 \|\| window > (\d+)\)")):
        m = re.findall(pattern, text, re.M)
        assert len(m) == 1, name
        out[name] = int(m[0])
    return out


_K = source_constants()
FIN_BLOCK, SUMMARY_HEAD = _K["FIN_BLOCK"], _K["MPPI_SUMMARY_HEAD"]
WAVE_ROLLOUT_MAX_T, SG_MAX_WINDOW = _K["WAVE_ROLLOUT_MAX_T"], _K["SG_MAX_WINDOW"]
WAVE_ROLLOUT_MODELS = ("racing", "racing_discs")  # is_racing_model: Model<RACING>::rollout_wave, inherited by the disc models


def sg_admitted(T, dc, window):
    """mppi_set_sg_filter's answer: 0 switches the filter off; else odd, <= 255, window / 2 <= 2T - 1, T * dc <= FIN_BLOCK."""
    if window == 0:
        return True
    return window > 0 and window % 2 == 1 and window <= SG_MAX_WINDOW and T * dc <= FIN_BLOCK and window // 2 <= 2 * T - 1


def history_rows(T):
    return T - 1


def history_alloc_floats(T, dc):
    return max(T - 1, 1) * dc


def staging_rounds(T, dc):
    """Passes of finalize_tail's staging loop `for (idx = threadIdx.x; idx < (2T - 1) * dc; idx += FIN_BLOCK)`."""
    return -(-(2 * T - 1) * dc // FIN_BLOCK)


def combine_rounds(row):
    """Passes of the combine's `for (cidx = threadIdx.x; cidx < row; cidx += FIN_BLOCK)`."""
    return -(-row // FIN_BLOCK)


def takes_wave_rollout(model, T, math):
    """batch1_rollout: `if constexpr (is_racing_model(MODEL) && FAST) { if (T <= 63) rollout_wave }`."""
    return model in WAVE_ROLLOUT_MODELS and math != 0 and T <= WAVE_ROLLOUT_MAX_T


def _rng(*key):
    return np.random.default_rng([zlib.crc32(repr(key).encode())])


# ------------------------------------------------------------------------------ 1. the filter table
def _filter_shapes():
    out = [(1, dc, w) for dc in (1, 2) for w in (1, 3)]                      # zero history rows
    out += [(2, dc, w) for dc in (1, 2, 4) for w in (3, 7)]                  # one history row; 7 is the widest admitted
    out += [(3, 1, 11)]                                                      # p = n = 5: the flip copies the whole sequence
    out += [(T, 2, w) for T in (5, 12) for w in (5, 9)]                      # ordinary shapes
    out += [(64, 1, 255), (128, 1, 255)]                                     # the cap and the horizon limit at once; the cap alone
    out += [(1024, 1, 5), (512, 2, 5), (256, 4, 9)]                          # row = FIN_BLOCK
    out += [(7, 3, 5), (170, 6, 9)]                                          # generic handles of 3 and 6 controls (row 1020)
    return tuple(out)


FILTER_SHAPES = _filter_shapes()
TAP_KINDS = ("savgol", "asymmetric")
HISTORY_KINDS = ("zero", "random")
FILTER_SOLVES = 3  # consecutive store_mean = 1 calls per handle: the history shifts twice under fresh rows
REFUSALS = (  # (T, dc, window): what mppi_set_sg_filter must refuse
    (5, 2, 4),       # even
    (200, 1, 257),   # odd, inside the horizon limit, above 255
    (2, 2, 9),       # window / 2 = 4 > 2T - 1 = 3
    (1025, 1, 3),    # row = FIN_BLOCK + 1
)


def savgol_order(window):
    """The reference's order 3 where the window allows it (window > order)."""
    return min(3, window - 1)


def taps(kind, T, dc, window):
    """fp32 taps [window].  savgol: the real coefficients (symmetric).  asymmetric: uniform on [-1, 1], no two entries equal —
    a reversed tap index, a mirrored staging read or swapped front / back padding changes the sum."""
    if kind == "savgol":
        from pi_mpc import _host

        return _host.savitzky_golay_coeffs(window, savgol_order(window))
    rng = _rng("taps", T, dc, window)
    while True:
        c = rng.uniform(-1.0, 1.0, window).astype(f32)
        if len(np.unique(c)) == window and (window == 1 or np.all(c[: window // 2] != c[::-1][: window // 2])):
            return c


def history(kind, T, dc):
    """[T - 1, dc] fp32: zeros (what the product starts from) or a caller's own."""
    if kind == "zero":
        return np.zeros((T - 1, dc), f32)
    return _rng("history", T, dc).uniform(-2.0, 2.0, (T - 1, dc)).astype(f32)


def filter_row(T, dc, window, k):
    """The action sequence [T, dc] injected at solve k of a filter case: both signs, no structure the filter could hide behind."""
    return _rng("row", T, dc, window, k).uniform(-2.0, 2.0, (T, dc)).astype(f32)


def one_shard(A):
    """The summary {min 0, sum e 1, sum e^2 1, sum e*c 0, A}: the tail's action is A bit for bit."""
    A = np.ascontiguousarray(A, f32).reshape(-1)
    return np.concatenate([f32([0.0, 1.0, 1.0, 0.0]), A])[None, :]


def convolve64(hist, A, c):
    """Step 7 written independently of pi_mpc._host, in float64: y = [history; A] per control, padded by p = len(c) // 2 mirrored
    samples at both ends (y[p - 1], ..., y[0] in front, y[n - 1], ..., y[n - p] behind), out[i] = sum_j c[j] * ypad[i + j];
    the last T rows."""
    hist, A, c = np.asarray(hist, f64), np.asarray(A, f64), np.asarray(c, f64)
    T, dc = A.shape
    y = np.concatenate([hist.reshape(-1, dc), A], axis=0)
    n, w = len(y), len(c)
    p = w // 2
    q = np.arange(n - T, n)[:, None] + np.arange(w)[None, :] - p   # [T, w]: index into y of tap j at output row t ...
    q = np.where(q < 0, -q - 1, np.where(q >= n, 2 * n - 1 - q, q))  # ... mirrored about the ends
    return np.einsum("j,tjk->tk", c, y[q])


# ------------------------------------------------------------------------------ 2. the shard table
Shard = namedtuple("Shard", "name T dc W lam summaries exact dead")  # summaries [W, 4 + T * dc] fp32; dead: shard indices


def _live_shards(rng, W, row, minima, integer=False):
    """W summaries with the given minima: positive sums, rows A_g = u * se_g with u in [1, 3] (every column bounded away from
    zero).  integer: se_g powers of two, every other entry a small integer — every sum the kernel forms is exact."""
    out = np.empty((W, SUMMARY_HEAD + row), f32)
    for g in range(W):
        if integer:
            se = f32(2.0 ** int(rng.integers(0, 4)))
            se2, sec = f32(rng.integers(1, 9)), f32(rng.integers(1, 9))
            u = rng.integers(1, 4, row).astype(f32)
        else:
            se, se2, sec = (f32(v) for v in rng.uniform(0.5, 4.0, 3))
            u = rng.uniform(1.0, 3.0, row).astype(f32)
        out[g, 0], out[g, 1], out[g, 2], out[g, 3] = minima[g], se, se2, sec
        out[g, SUMMARY_HEAD:] = u * se
    return out


def _with_dead(live, where, lam):
    """One more shard at `where`: minimum DEAD_GAP * lambda (and a little) above the largest live one, everything else 1e30."""
    dead = np.full((1, live.shape[1]), DEAD_VALUE, f32)
    dead[0, 0] = f32(float(live[:, 0].max()) + 1.5 * DEAD_GAP * lam)
    return np.concatenate([live[:where], dead, live[where:]], axis=0)


ROW_SHAPES = ((1, 1), (1, 3), (4, 1), (5, 1), (341, 3), (1024, 1), (1025, 1), (417, 6))  # rows 1, 3, 4, 5, 1023, 1024, 1025, 2502
SHARD_COUNTS = (1, 2, 3, 8, 64)
BASE_ROW = (5, 2)


def _shard_cases():
    out = []

    def add(name, T, dc, W, lam, summaries, exact=False, dead=()):
        assert summaries.shape == (W, SUMMARY_HEAD + T * dc) and summaries.dtype == f32
        out.append(Shard(name, T, dc, W, float(lam), summaries, exact, tuple(dead)))

    T, dc = BASE_ROW
    row = T * dc
    for W in SHARD_COUNTS:
        rng = _rng("shards", W)
        # equal minima, powers of two, integers: f = 1 and every sum is exact
        add(f"equal_W{W}", T, dc, W, 0.7, _live_shards(rng, W, row, np.full(W, 3.5, f32), integer=True), exact=True)
        # gaps of a few lambda
        lam = 0.8
        add(f"dense_W{W}", T, dc, W, lam, _live_shards(rng, W, row, (2.0 + lam * rng.uniform(0.0, 4.0, W)).astype(f32)))
        if W > 1:
            # minima of both signs
            m = (lam * rng.uniform(-3.0, 3.0, W)).astype(f32)
            m[0], m[-1] = -abs(m[0]) - f32(0.1), abs(m[-1]) + f32(0.1)
            add(f"signs_W{W}", T, dc, W, lam, _live_shards(rng, W, row, m))
            # a common offset of 1e6 (fp32 spacing 1 / 16), unit spread
            add(f"offset_W{W}", T, dc, W, 1.0, _live_shards(rng, W, row, (1.0e6 + rng.uniform(0.0, 3.0, W)).astype(f32)))
            # one shard 87 / 88 lambda above the minimum: f = 1.6e-38 / 6.1e-39, either side of FLT_MIN = 1.18e-38
            for gap in (87.0, 88.0):
                m = (5.0 + lam * rng.uniform(0.0, 3.0, W)).astype(f32)
                m[(int(np.argmin(m)) + 1) % W] = f32(float(m.min()) + gap * lam)
                add(f"gap{int(gap)}_W{W}", T, dc, W, lam, _live_shards(rng, W, row, m))
    # W = 1 with se = 1: a = A to the bit, whatever A holds
    rng = _rng("w1")
    s = _live_shards(rng, 1, row, f32([1.25]))
    s[0, 1] = 1.0
    s[0, SUMMARY_HEAD:] = rng.uniform(-3.0, 3.0, row).astype(f32)
    add("w1_se1", T, dc, 1, 0.3, s, exact=True)
    # dead shards: first, last, in the middle; among 1, 2, 7 and 63 live ones
    for L in (1, 2, 7, 63):
        rng = _rng("dead", L)
        lam = 0.5
        live = _live_shards(rng, L, row, (1.0 + lam * rng.uniform(0.0, 4.0, L)).astype(f32))
        for label, where in (("first", 0), ("last", L), ("middle", (L + 1) // 2)):
            if L == 1 and label == "middle":
                continue
            add(f"dead_{label}_L{L}", T, dc, L + 1, lam, _with_dead(live, where, lam), dead=(where,))
    # two dead shards, an equal-minima live set: exact AND dead
    rng = _rng("dead_equal")
    live = _live_shards(rng, 3, row, np.full(3, -2.0, f32), integer=True)
    both = _with_dead(_with_dead(live, 3, 1.0), 0, 1.0)
    add("dead_both_ends_equal", T, dc, 5, 1.0, both, exact=True, dead=(0, 4))
    # every row shape, dense, three shards (and the long list on the longest row)
    for T, dc in ROW_SHAPES:
        rng = _rng("rows", T, dc)
        add(f"row{T * dc}_T{T}_dc{dc}", T, dc, 3, 1.0, _live_shards(rng, 3, T * dc, (4.0 + rng.uniform(0.0, 3.0, 3)).astype(f32)))
    T, dc = ROW_SHAPES[-1]
    rng = _rng("rows64")
    add(f"row{T * dc}_W64", T, dc, 64, 1.0, _live_shards(rng, 64, T * dc, (4.0 + rng.uniform(0.0, 3.0, 64)).astype(f32)))
    T, dc = 341, 3
    live = _live_shards(_rng("rows_dead"), 2, T * dc, f32([0.5, 1.0]))
    add("row1023_dead_middle", T, dc, 3, 1.0, _with_dead(live, 1, 1.0), dead=(1,))
    return tuple(out)


SHARD_CASES = _shard_cases()


def shard_case(name):
    for c in SHARD_CASES:
        if c.name == name:
            return c
    raise KeyError(name)


def combine_argument(minima, lam):
    """The fp32 argument the kernel hands to expf: fl(fl(-m_g / lambda) - x_max), x_max = max_g fl(-m_g / lambda)."""
    x = ((-np.asarray(minima, f32)) / f32(lam)).astype(f32)
    return (x - x.max()).astype(f32)


def combine_reference(summaries, lam):
    """(cmin, se, se2, sec, a[row]): float64 over the fp32 argument the kernel forms (the `weights64` convention): exp and
    everything after it in float64.  Shards of factor exactly 0 are left out."""
    s = np.asarray(summaries, f32)
    f = np.exp(combine_argument(s[:, 0], lam).astype(f64))
    live = f != 0.0
    f, s64 = f[live], s[live].astype(f64)
    se = float(f @ s64[:, 1])
    return (f32(s[:, 0].min()), se, float((f * f) @ s64[:, 2]), float(f @ s64[:, 3]), (f @ s64[:, SUMMARY_HEAD:]) / se)


def combine_fp32(summaries, lam):
    """The same combine in sequential fp32 without fused multiply-adds (W terms per sum, numpy's expf, one quotient): an
    equally valid evaluation, which the host test holds to the GPU test's limit of the float64 reference."""
    s = np.asarray(summaries, f32)
    f = np.exp(combine_argument(s[:, 0], lam)).astype(f32)
    se = se2 = sec = f32(0.0)
    a = np.zeros(s.shape[1] - SUMMARY_HEAD, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in range(len(s)):
            if f[g] == 0.0:
                continue  # (0 * 1e30 = 0: adding it changes nothing)
            se = f32(se + f32(f[g] * s[g, 1]))
            se2 = f32(se2 + f32(f32(f[g] * f[g]) * s[g, 2]))
            sec = f32(sec + f32(f[g] * s[g, 3]))
            a = (a + (f[g] * s[g, SUMMARY_HEAD:]).astype(f32)).astype(f32)
    return f32(s[:, 0].min()), se, se2, sec, (a / se).astype(f32)


def combine_exact(summaries):
    """Exact cases (equal minima, or W = 1 with se = 1): every factor is 1 and every sum is exact in fp32, so the result is the
    correctly rounded quotient of exact sums: fp32 bits."""
    s = np.asarray(summaries, f32)
    live = s[:, 0] == s[:, 0].min()
    assert np.all(s[~live, 1] == f32(DEAD_VALUE))
    tot = s[live].astype(f64).sum(axis=0)
    assert np.all(tot == tot.astype(f32).astype(f64)) and np.all(np.abs(tot) < 2.0 ** 24)
    se = f32(tot[1])
    return f32(s[:, 0].min()), se, f32(tot[2]), f32(tot[3]), (tot[SUMMARY_HEAD:].astype(f32) / se).astype(f32)


def without_dead(case):
    return np.delete(case.summaries, list(case.dead), axis=0)


def permutations(W):
    """Orders of the live shards the combine must not care about beyond rounding: reversed, and one shuffle."""
    if W < 2:
        return []
    out = [np.arange(W)[::-1]]
    p = _rng("perm", W).permutation(W)
    if W > 2 and not np.array_equal(p, np.arange(W)) and not np.array_equal(p, out[0]):
        out.append(p)
    return out


# ------------------------------------------------------------------------------ 3. the batch-1 table
B1_HORIZONS = {"racing": (1, 2, 3, 62, 63, 64, 65), "racing_discs": (1, 2, 3, 62, 63, 64, 65),
               "nav2d": (1, 2, 15), "pendulum": (1, 2, 15), "cartpole": (1, 2, 15)}
B1_CASES = tuple((m, T) for m, Ts in B1_HORIZONS.items() for T in Ts)
B1_MATHS = (0, 1, 2)
B1_DEFAULT_MATH = 2          # mppi_handle.hpp: `int math_fast = 2;`
B1_SAMPLES = 256
B1_DC = {"racing": 2, "racing_discs": 2, "nav2d": 2, "pendulum": 1, "cartpole": 1}
B1_LIMITS = {  # (u_min, u_max): helpers.MODEL_CFG; racing_discs_ref.U_MIN / U_MAX
    "racing": ([-2.0, -0.25], [2.0, 0.25]), "racing_discs": ([-2.0, -0.25], [2.0, 0.25]),
    "nav2d": ([0.0, -1.0], [2.0, 1.0]), "pendulum": ([-2.0], [2.0]), "cartpole": ([-3.0], [3.0]),
}
B1_HEADING = {"racing": 2, "racing_discs": 2, "nav2d": 2}  # EntryGeneral models: any finite heading, row 0 keeps the caller's
B1_DISC_TABLES = ("n0", "n3")  # racing_discs_ref.CASES: an empty table, three discs crossing the path
B1_ACTION_KINDS = ("inside", "outside")


def b1_actions(model, T, kind):
    """[T, dc] fp32.  inside: uniform within the control bounds.  outside: uniform over 1.6 x the bounds' span around their
    centre, step 0 pinned beyond u_max and the last step beyond u_min — the model's step clamps them, the wave path again."""
    lo, hi = (np.asarray(v, f64) for v in B1_LIMITS[model])
    rng = _rng("b1", model, T, kind)
    if kind == "inside":
        return rng.uniform(lo, hi, (T, len(lo))).astype(f32)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    A = rng.uniform(mid - 1.6 * half, mid + 1.6 * half, (T, len(lo)))
    A[0] = hi + 0.25 * half
    if T > 1:
        A[-1] = lo - 0.25 * half
    return A.astype(f32)


def b1_starts(model, base):
    """[base] and, for the models that take any finite heading, base with the heading two turns and a little on."""
    out = [np.asarray(base, f32).copy()]
    if model in B1_HEADING:
        y = out[0].copy()
        j = B1_HEADING[model]
        y[j] = f32(y[j] + f32(4.0 * np.pi) + f32(0.03))
        assert abs(float(y[j])) > np.pi
        out.append(y)
    return out


def b1_base_start(model):
    """The suite's usual start of a model (racing_discs: chosen by racing_discs_ref.case in the GPU test)."""
    if model == "racing":
        from helpers import racing_env_fixture

        return np.asarray(racing_env_fixture()["start_state"], f32)
    return f32({"pendulum": [3.0, 0.1], "cartpole": [0.01, 0.0, 0.02, 0.0], "nav2d": [-9.0, -9.0, 0.785]}[model])
