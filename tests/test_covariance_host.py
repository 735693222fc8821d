"""Covariance adaptation, the parts that need no GPU: the scalar update rule of csrc/mppi_covariance.hpp (the text the device
kernel compiles, built here with g++) against numpy, and the validation of the MPPI keyword arguments."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mppi_playground_amd", "csrc", "mppi_covariance.hpp")


@pytest.fixture(scope="module")
def step(tmp_path_factory):
    """covariance_step over arrays, from a shared object this test builds from the product's header."""
    d = tmp_path_factory.mktemp("covariance_step")
    src = d / "step.cpp"
    src.write_text(
        '#include "%s"\n'
        'extern "C" void step_n(const float* s2, const float* var, const float* rate, const float* floor,\n'
        "                       const float* smin, const float* smax, int n, float* out) {\n"
        "    for (int i = 0; i < n; ++i) out[i] = mppi::covariance_step(s2[i], var[i], rate[i], floor[i], smin[i], smax[i]);\n"
        "}\n" % HEADER)
    so = d / "libstep.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.step_n.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    lib.step_n.restype = None

    def run(*cols):
        cols = [np.ascontiguousarray(c, np.float32) for c in cols]
        out = np.empty(len(cols[0]), np.float32)
        lib.step_n(*[c.ctypes.data_as(C.c_void_p) for c in cols], len(out), out.ctypes.data_as(C.c_void_p))
        return out

    return run


def numpy_step(s2, var, rate, floor, smin, smax):
    """The rule of the issue in fp32, one rounding per operation: s^2 <- (1 - a) s^2 + a (var + floor), s clamped."""
    f = np.float32
    s2, var, rate, floor, smin, smax = (np.asarray(a, f) for a in (s2, var, rate, floor, smin, smax))
    target = (var + floor).astype(f)
    new = (((f(1.0) - rate).astype(f) * s2).astype(f) + (rate * target).astype(f)).astype(f)
    return np.minimum(np.maximum(np.sqrt(new).astype(f), smin), smax).astype(f)


def _grid():
    f = np.float32
    sig = np.array([0.0, 1e-3, 0.1, 0.5, 1.0, 3.0], f)
    var = np.array([0.0, 1e-12, 1e-6, 2.5e-3, 0.25, 1.0, 17.0], f)
    rate = np.array([0.0, 0.5, 1.0, 0.123], f)
    floor = np.array([0.0, 1e-6, 1e-2], f)
    lim = [(0.0, np.inf), (0.05, np.inf), (0.0, 0.7), (0.2, 0.4), (5.0, 6.0)]  # (5, 6): smin > sqrt(var + floor) for most of the grid
    rows = [(s * s, v, r, fl, lo, hi) for s in sig for v in var for r in rate for fl in floor for lo, hi in lim]
    return [np.array(c, f) for c in zip(*rows)]


def test_covariance_step_equals_numpy_on_a_grid(step):
    cols = _grid()
    got, want = step(*cols), numpy_step(*cols)
    assert np.array_equal(got, want)
    assert np.all(np.isfinite(got))
    s2, var, rate, floor, smin, smax = cols
    assert np.all(got >= smin) and np.all(got <= smax)


def test_rate_zero_never_moves_and_rate_one_is_the_sketch(step):
    f = np.float32
    rng = np.random.default_rng(3)
    s = np.concatenate([rng.uniform(1e-3, 4.0, 4000), [0.1, 0.5, 1.0, 0.25]]).astype(f)
    n = len(s)
    var = rng.uniform(0.0, 3.0, n).astype(f)
    zero, one, inf = np.zeros(n, f), np.ones(n, f), np.full(n, np.inf, f)
    floor = np.full(n, 1e-6, f)
    # rate 0: sqrt(fl(s * s)) is s itself, bit for bit (what keeps a solver with cov_rate = 0 on today's noise)
    assert np.array_equal(step((s * s).astype(f), var, zero, floor, zero, inf), s)
    # rate 1: the reference's sketch, covariance = var + small_cov (mppi.py:402-411), whatever the old entry was
    assert np.array_equal(step((s * s).astype(f), var, one, floor, zero, inf), np.sqrt((var + floor).astype(f)).astype(f))
    # var = 0 (one sample carries all the weight): sqrt(floor), or sigma_min where that is larger
    assert np.array_equal(step((s * s).astype(f), zero, one, floor, zero, inf), np.full(n, np.sqrt(f(1e-6)), f))
    assert np.array_equal(step((s * s).astype(f), zero, one, floor, np.full(n, 0.05, f), inf), np.full(n, 0.05, f))


def test_keyword_validation():
    from pi_mpc import _host  # (tests/conftest.py imports mppi_playground_amd, which puts pi_mpc/ on the path)

    ok = dict(adapt_covariance=True, cov_rate=0.5, cov_floor=1e-6, sigma_min=None, sigma_max=None, dim_control=2,
              shard_samples=False, noise_source="philox")
    rate, floor, smin, smax = _host.check_covariance_args(**ok)
    assert (rate, floor) == (0.5, 1e-6) and np.array_equal(smin, [0.0, 0.0]) and np.all(np.isinf(smax))
    for bad in (dict(cov_rate=-0.1), dict(cov_rate=1.5), dict(cov_rate=float("nan")), dict(cov_floor=-1e-9),
                dict(sigma_min=np.array([0.1, 0.5]), sigma_max=np.array([0.2, 0.4])), dict(sigma_min=np.array([-0.1, 0.0])),
                dict(sigma_min=np.array([0.1])), dict(shard_samples=True), dict(noise_source="torch_cpu")):
        with pytest.raises(ValueError):
            _host.check_covariance_args(**dict(ok, **bad))
    # the two exclusions only bind when the adaptation is asked for
    _host.check_covariance_args(**dict(ok, adapt_covariance=False, shard_samples=True, noise_source="torch_cpu"))
