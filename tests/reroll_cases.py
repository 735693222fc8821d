"""The case tables of the re-roll tests (tests/test_gpu_reroll.py on an MI355X, tests/test_reroll_cases_host.py without one).

Five device code paths rebuild a sample's state trajectory after a solve (csrc/mppi_topk.hpp, mppi_finalize.hpp):
rollout_samples_kernel (`_state_seq_batch`), rollout_actions_kernel (explicit actions) and topk_rollout_kernel in its three
launches (direct: the block sorts the costs itself; select: fed by the radix select; sorted: k > 1024, a candidate per thread).
The cases below are the smallest that take every branch of rollout_states_noise and every launch, for every native model:

  horizons   dc = 1 (four steps per float4 group): T = 1, 2, 3, 4, 5, 7, 8 — 0, 1 and 2 whole groups, remainders 1, 2, 3, 0;
             dc = 2: T = 1 .. 5; and the two sides of TopkLds::PREGEN_MAX_R = 32 groups per row (T = 128 / 129 for dc = 1,
             64 / 65 for dc = 2), whose second horizon also ends in a partial group;
  samples    N = 200 with exploration = 0.25: the split at 150 falls inside tile 2 and the last tile is ragged;
             k = 1, 64, 65, 200; plus N = 4160 / k = 65 (select) and N = 1100 / k = 1100 (sorted) for two models;
  starts     the suite's usual ones; the models that accept any finite heading (EntryGeneral: nav2d, racing) get a second
             start whose heading lies outside [-pi, pi];
  redo       the starts of test_extreme_initial_states_against_oracle that leave the fast paths, at T = 5 and 25, N = 192.

Everything here runs on the host: the oracle (and tests/mlp_ref.py for the learned models) on philox_normal noise gives each
case's cost scale, from which the case's temperature is chosen (see `temperature`), and the reference's own sensitivity
(`ulp_probe`)."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

import mlp_ref
from helpers import MODEL_CFG, goalzone_env_fixture, oracle_problem, orc, racing_env_fixture

f32, f64 = np.float32, np.float64
TOL = 1e-5          # the suite's limit (test_gpu_parity.TOL): states against the oracle, weights against float64
REDO_TOL = 1e-4     # test_extreme_initial_states_against_oracle's own limit: the conditioning of those starts
SEED, SOLVE_IDX = 42, 5   # MPPI's default seed; the solve index every case draws its noise at
EXPLORATION = 0.25
N_BASE, KS = 200, (1, 64, 65, 200)
MATHS = (0, 1, 2)
NOISE_SOURCES = ("regen", "tiles", "inject")
PREGEN_MAX_R, TOPK_MAX, TOPK_DIRECT_MAX, WAVE = 32, 1024, 4096, 64  # csrc/mppi_lds.hpp, mppi_topk.hpp

NATIVE = ("pendulum", "cartpole", "mountaincar", "mjcartpole", "nav2d", "racing", "goalzone")
MLP = {"mlp41": "mlp41_relu_2l_res", "mlp42": "mlp42_relu_2l_abs"}  # relu: option math = 0 is the fp32 restatement bit for bit
MODELS = NATIVE + tuple(MLP)
DC = {"pendulum": 1, "cartpole": 1, "mountaincar": 1, "mjcartpole": 1, "nav2d": 2, "racing": 2, "goalzone": 2, "mlp41": 1, "mlp42": 2}
HORIZONS = {1: (1, 2, 3, 4, 5, 7, 8), 2: (1, 2, 3, 4, 5)}
BOUNDARY = {"pendulum": (128, 129), "cartpole": (128, 129), "nav2d": (64, 65), "racing": (64, 65)}
LAUNCH_MODELS = (("pendulum", 5), ("nav2d", 3))
LAUNCH_SHAPES = ((4160, (65,)), (1100, (1100,)))
HEADING = {"nav2d": 2, "racing": 2, "goalzone": 2}   # the component the model stores wrapped to [-pi, pi)
ENTRY_GENERAL = ("nav2d", "racing")                     # csrc/mppi_models.inc: ENTRY_GENERAL
ROW0_MUTATED = ("mountaincar",)  # its dynamics mutates the input views (oracle/mppi_oracle.c: ss != s): row 0 is not x0

Case = namedtuple("Case", "name model T N ks")
Redo = namedtuple("Redo", "name model T N ks x0")


def _cases():
    out = []
    for m in MODELS:
        for T in HORIZONS[DC[m]] + BOUNDARY.get(m, ()):
            out.append(Case(f"{m}_T{T}", m, T, N_BASE, KS))
    for m, T in LAUNCH_MODELS:
        for N, ks in LAUNCH_SHAPES:
            out.append(Case(f"{m}_T{T}_N{N}", m, T, N, ks))
    return tuple(out)


CASES = _cases()
REDO_STARTS = (("pendulum", (-9.9e4, 7.9)), ("pendulum", (1.2e5, -8.0)), ("cartpole", (1.0, 0.0, 1e4, 2.0)),
               ("mjcartpole", (0.1, 0.2, 5e3, 0.0)))
REDO_CASES = tuple(Redo(f"{m}_redo{i}_T{T}", m, T, 192, (1, 64, 65, 192), x0)
                   for i, (m, x0) in enumerate(REDO_STARTS) for T in (5, 25))
REDO_MATHS = (1, 2)


# ------------------------------------------------------------------------------ geometry, from the table alone
def geometry(model, T, N, k, noise="regen"):
    """What the kernels derive from a case: R = ceil(T * dc / 4) float4 groups per row (the formula test_lds_layouts_host.py
    restates), steps per group, whole groups and remainder of rollout_states_noise, the launch mppi_top_samples picks and
    TopkLds::pregen."""
    dc = DC[model]
    R, spg = (T * dc + 3) // 4, 4 // dc
    launch = "sorted" if k > TOPK_MAX else ("direct" if N <= TOPK_DIRECT_MAX else "select")
    thr = int(N * (1 - EXPLORATION))
    return dict(R=R, spg=spg, gfull=T // spg, rem=T % spg, launch=launch,
                pregen=launch != "sorted" and noise == "regen" and R <= PREGEN_MAX_R,
                split_inside_tile=thr % WAVE != 0 and 0 < thr < N, ragged_last_tile=N % WAVE != 0, threshold=thr)


# ------------------------------------------------------------------------------ inputs
def float_to_key(c):
    """csrc/mppi_common.hpp float_to_key: unsigned order = float order, -0.0 before +0.0."""
    b = np.ascontiguousarray(c, dtype=f32).view(np.uint32)
    return np.where((b & np.uint32(0x80000000)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def host_order(costs):
    """(order, keys): the stable sort of (cost key, index) — the words the device sorts."""
    keys = float_to_key(costs)
    return np.lexsort((np.arange(len(keys)), keys)), keys


def order_is_determined(keys, order, k, launch):
    """Ties INSIDE the first k are ordered by index on every launch (the candidates are sorted as (key << 32) | index words).
    Only the radix select of the `select` launch takes ties AT the k-th key in the order its atomics meet them: there the
    k-th and the (k + 1)-th key must differ."""
    if launch != "select" or k >= len(keys):
        return True
    return bool(keys[order[k - 1]] != keys[order[k]])


def limits(model):
    """(u_min, u_max, sigmas) as float32 rows."""
    cfg = mlp_ref.LIMITS[DC[model]] if model in MLP else MODEL_CFG[model]
    return tuple(np.asarray(cfg[k], f32) for k in ("u_min", "u_max", "sigmas"))


def starts(model):
    """The start states of a model's cases: the suite's usual one, then (EntryGeneral models) one whose heading is outside
    [-pi, pi]."""
    if model in MLP:
        return [mlp_ref.X0.copy()]
    if model == "racing":
        x = np.asarray(racing_env_fixture()["start_state"], f32)
    elif model == "goalzone":
        x = np.asarray(goalzone_env_fixture()["x0"], f32)
    else:
        x = f32({"pendulum": [3.0, 0.1], "cartpole": [0.01, 0.0, 0.02, 0.0], "mountaincar": [-0.5, 0.0],
                 "mjcartpole": [0.0, 0.0, 0.05, 0.0], "nav2d": [-9.0, -9.0, 0.785]}[model])
    out = [x]
    if model in ENTRY_GENERAL:
        y = x.copy()
        y[HEADING[model]] = f32(y[HEADING[model]] + f32(4.0 * np.pi) + f32(0.03))  # two turns on, not a multiple of 2 pi away
        assert abs(float(y[HEADING[model]])) > np.pi
        out.append(y)
    return out


def warm_start(name, T, dc):
    """The random mean a case samples around (scale 0.25, like the neighbouring tests' 0.2 .. 0.3)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return (rng.standard_normal((T, dc)) * 0.25).astype(f32)


@lru_cache(maxsize=None)
def racing_reference(T):
    """The reference window of the racing cases, from the environment's start state as in test_edge_sizes_against_oracle
    (host arithmetic only: test_host_logic.test_calc_ref_trajectory)."""
    import torch
    from envs.racing_controller import racing_controller

    env = _racing_env()
    ctrl = racing_controller.__new__(racing_controller)
    ctrl.env = env
    ref, _ = ctrl.calc_ref_trajectory(torch.from_numpy(np.asarray(racing_env_fixture()["start_state"], f32)),
                                      env.racing_center_path, 0, T, DL=0.1, lookahead_distance=3, reference_path_interval=0.85)
    return ref.numpy().copy()


@lru_cache(maxsize=None)
def _racing_env():
    from envs.racing_env import RacingEnv

    return RacingEnv(device="cpu")


def problem(model, T, N, exploration=EXPLORATION):
    P = oracle_problem(model, N, T, exploration)
    if model == "racing":
        P.set_ref_path(racing_reference(T))
    return P


@lru_cache(maxsize=None)
def mlp_case(model):
    return mlp_ref.case(MLP[model])


def clamped_actions(model, mean, eps, N):
    """clamp(mean + eps) with the zero mean beyond the exploration split (mppi.py:266-275), fp32."""
    u_min, u_max, _ = limits(model)
    thr = int(N * (1 - EXPLORATION))
    U = eps.astype(f32).copy()
    U[:thr] = (mean[None] + eps[:thr]).astype(f32)
    return np.minimum(np.maximum(U, u_min), u_max).astype(f32)


def reference_states(model, T, N, x0, mean, eps, U=None, dtype=f32):
    """(costs, S) of a solve's samples: the oracle for the native models, tests/mlp_ref.py (on the clamped actions) for the
    learned ones."""
    if model in MLP:
        cs = mlp_case(model)
        U = clamped_actions(model, mean, eps, N) if U is None else U
        c, S, _ = mlp_ref.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], x0, U, dtype)
        return c, S
    r = problem(model, T, N).rollout_cost(x0, mean, eps, want_S=True)
    return r["costs"], r["S"]


def state_error(model, got, want):
    """max |got - want| / max |want| with the wrapped heading's difference taken modulo 2 pi."""
    d = np.abs(np.asarray(got, f64) - np.asarray(want, f64))
    if model in HEADING:
        j = HEADING[model]
        d[..., j] = np.minimum(d[..., j], np.abs(2.0 * np.pi - d[..., j]))
    return float(d.max() / max(np.abs(np.asarray(want, f64)).max(), 1e-30))


def temperature(costs):
    """The case's temperature.  The device forms a weight as expf(fl(-c / lambda) - fl(-cmin / lambda)) / sum: each fp32
    quotient is off by up to 2^-24 |c| / lambda, so the weight is off by about 2^-23 max|c| / lambda of itself before expf and
    the sum add their few 1e-7.  max|c| / lambda <= 32 keeps that under 4e-6 + 1e-6 < TOL for a comparison with the float64
    softmax; lambda is the next power of two above max|c| / 32 (at least 1)."""
    m = float(np.abs(np.asarray(costs, f64)).max())
    return float(2.0 ** max(0, int(np.ceil(np.log2(max(m, 1e-30) / 32.0)))))


@lru_cache(maxsize=None)
def host_solve(name, model, T, N, start):
    """What the host alone knows of case `name` at start number `start`: x0, mean, philox_normal noise (the device's draw to
    1e-4 of sigma), the reference's costs and the temperature chosen from them."""
    _, _, sig = limits(model)
    x0 = tuple(starts(model))[start] if isinstance(start, int) else f32(start)
    mean = warm_start(name, T, DC[model])
    eps = orc.philox_normal(SEED, SOLVE_IDX, 0, N, T, DC[model], sig)
    costs, _ = reference_states(model, T, N, x0, mean, eps)
    return dict(x0=x0, mean=mean, eps=eps, costs=costs, lam=temperature(costs))


# ------------------------------------------------------------------------------ the reference's own sensitivity
def ulp_probe(model, T, rows=64, seed=0):
    """How far the reference's states move when every action moves by one fp32 ulp: 64 random clamped action rows, each
    action stepped to a neighbouring float (direction at random, kept inside the bounds), as a fraction of max|S|."""
    rng = np.random.default_rng(seed + 1000 * T + zlib.crc32(model.encode()) % 1000)
    u_min, u_max, sig = limits(model)
    dc = DC[model]
    U = np.minimum(np.maximum((rng.standard_normal((rows, T, dc)) * sig).astype(f32), u_min), u_max).astype(f32)
    up = rng.random(U.shape) < 0.5
    V = np.where(up, np.nextafter(U, f32(np.inf)), np.nextafter(U, f32(-np.inf))).astype(f32)
    V = np.minimum(np.maximum(V, u_min), u_max).astype(f32)
    x0 = starts(model)[0]
    zero = np.zeros((T, dc), f32)
    if model in MLP:
        _, A = reference_states(model, T, rows, x0, zero, U, U=U)
        _, B = reference_states(model, T, rows, x0, zero, V, U=V)
    else:
        P = problem(model, T, rows, exploration=0.0)
        A = P.rollout_cost(x0, zero, U, want_S=True)["S"]
        B = P.rollout_cost(x0, zero, V, want_S=True)["S"]
    return state_error(model, B, A)
