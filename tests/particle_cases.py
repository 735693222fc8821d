"""Cost matrices [P, N] for the tests of the particle fold (tests/test_particles_host.py, tests/test_gpu_particles.py), and the
float64 evaluation the fp32 restatement (pi_mpc._host.fold_particle_costs) is held to."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
SIZES_N = (1, 63, 64, 65, 300)
SIZES_P = (1, 2, 3, 5, 8, 16)
MODES = ("mean", "worst", "cvar")
KINDS = ("ties", "dominant", "mixed", "magnitudes")


def ks(P):
    """The CVaR orders every case runs: 1 (the worst case), ceil(P / 4) and P (the descending-order mean)."""
    return sorted({1, math.ceil(P / 4), P})


def matrix(kind, P, N, seed=0):
    """[P, N] fp32, finite.
    ties: values from a set of five, so that most samples repeat a value among their particles;
    dominant: one particle (P // 2) far above the others; mixed: both signs; magnitudes: 1e-3 .. 1e6, signed."""
    rng = np.random.default_rng(1000 * seed + 17 * P + N)
    if kind == "ties":
        m = rng.choice(f32([-2.5, 0.125, 0.125, 3.0, 1e3]), (P, N))
    elif kind == "dominant":
        m = rng.uniform(0.0, 10.0, (P, N))
        m[P // 2] += 1.0e4
    elif kind == "mixed":
        m = rng.normal(0.0, 50.0, (P, N))
    elif kind == "magnitudes":
        m = rng.choice([-1.0, 1.0], (P, N)) * 10.0 ** rng.uniform(-3.0, 6.0, (P, N))
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(m, f32)


def fold64(m, mode, k=1):
    """The risk measure in float64 (exact sums of fp32 values up to one rounding each)."""
    m = np.asarray(m, f64)
    if mode == "mean":
        return m.sum(0) / m.shape[0]
    if mode == "worst":
        return m.max(0)
    s = -np.sort(-m, axis=0)
    return s[:k].sum(0) / k


def bound64(m, mode, k=1):
    """First-order bound of the fp32 fold against float64: a sequential sum of n addends rounds n - 1 times, the quotient
    once — n * 2^-24 of sum |c| over the addends (the maximum is exact)."""
    a = np.abs(np.asarray(m, f64))
    if mode == "worst":
        return np.zeros(a.shape[1])
    if mode == "mean":
        return a.shape[0] * 2.0 ** -24 * a.sum(0) / a.shape[0]
    s = -np.sort(-np.asarray(m, f64), axis=0)
    return k * 2.0 ** -24 * np.abs(s[:k]).sum(0) / k
