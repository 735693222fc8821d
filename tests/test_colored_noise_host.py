"""Temporally correlated sampling noise (noise_beta), the parts that need no GPU: the scalar rule of csrc/mppi_colored.hpp (the
text the device kernels compile, built here with g++) against a numpy restatement, the stationarity of that restatement, and
the validation of the MPPI keyword argument."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mppi_playground_amd", "csrc", "mppi_colored.hpp")
f32 = np.float32


def alpha_of(beta):
    """alpha as the library forms it: from the fp32 beta, square root in double, rounded once."""
    return f32(np.sqrt(1.0 - np.float64(f32(beta)) * np.float64(f32(beta))))


def restate(xi, beta):
    """z[..., T] from standard normals xi[..., T] (the chain runs along the last axis): z[0] = xi[0],
    z[t] = fl(fl(beta z[t-1]) + fl(alpha xi[t])), every product and the sum rounded to float32."""
    xi = np.asarray(xi, f32)
    b, a = f32(beta), alpha_of(beta)
    z = np.empty_like(xi)
    z[..., 0] = xi[..., 0]
    for t in range(1, xi.shape[-1]):
        z[..., t] = ((b * z[..., t - 1]).astype(f32) + (a * xi[..., t]).astype(f32)).astype(f32)
    return z


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    """(filter rows in place, alpha) from a shared object this test builds from the product's header."""
    d = tmp_path_factory.mktemp("colored_rule")
    src = d / "rule.cpp"
    src.write_text(
        '#include "%s"\n'
        'extern "C" float alpha_of(float beta) { return mppi::colored_alpha(beta); }\n'
        'extern "C" void filter_rows(float* x, int n, int T, float beta) {\n'
        "    const float alpha = mppi::colored_alpha(beta);\n"
        "    for (int i = 0; i < n; ++i)\n"
        "        for (int t = 1; t < T; ++t) x[i * T + t] = mppi::colored_step(x[i * T + t - 1], x[i * T + t], beta, alpha);\n"
        "}\n" % HEADER)
    so = d / "librule.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.alpha_of.argtypes, lib.alpha_of.restype = [C.c_float], C.c_float
    lib.filter_rows.argtypes, lib.filter_rows.restype = [C.c_void_p, C.c_int, C.c_int, C.c_float], None

    def run(xi, beta):
        x = np.array(xi, f32, order="C", copy=True)
        lib.filter_rows(x.ctypes.data_as(C.c_void_p), x.shape[0], x.shape[1], float(f32(beta)))
        return x

    return run, lambda beta: f32(lib.alpha_of(float(f32(beta))))


@pytest.mark.parametrize("T", [1, 2, 5, 64])
@pytest.mark.parametrize("beta", [1e-3, 0.5, 0.9, 0.999])
def test_header_equals_numpy(rule, T, beta):
    run, alpha = rule
    xi = np.random.default_rng(1000 * T + int(beta * 1000)).standard_normal((4096, T)).astype(f32)
    assert alpha(beta) == alpha_of(beta)
    got = run(xi, beta)
    assert np.array_equal(got, restate(xi, beta))
    assert np.array_equal(got[:, 0], xi[:, 0])  # the start is xi itself
    assert np.all(np.isfinite(got))


@pytest.mark.parametrize("beta", [0.5, 0.9, 0.99])
def test_restatement_is_stationary(beta):
    """Every step keeps variance 1 and the lag-1 correlation is beta, to six standard deviations of the two estimators over
    N independent samples: sqrt(2 / N) for mean z^2, sqrt((1 + beta^2) / N) for mean z[t] z[t-1]."""
    N, T = 65536, 8
    z = restate(np.random.default_rng(7).standard_normal((N, T)).astype(f32), beta).astype(np.float64)
    var_lim, cor_lim = 6.0 * np.sqrt(2.0 / N), 6.0 * np.sqrt((1.0 + beta * beta) / N)
    for t in range(T):
        dv = abs(np.mean(z[:, t] ** 2) - 1.0)
        dc = abs(np.mean(z[:, t] * z[:, t - 1]) - beta) if t else 0.0
        print(f"[colored] beta {beta} t {t}: |var - 1| {dv:.4f} (limit {var_lim:.4f}), |corr - beta| {dc:.4f} (limit {cor_lim:.4f})")
        assert dv <= var_lim
        assert dc <= cor_lim


def test_keyword_validation():
    from pi_mpc import _host  # (tests/conftest.py imports mppi_playground_amd, which puts pi_mpc/ on the path)
    import torch

    assert np.array_equal(_host.check_noise_beta_args(0.0, 2), f32([0.0, 0.0]))
    assert np.array_equal(_host.check_noise_beta_args(0.9, 3), f32([0.9, 0.9, 0.9]))
    assert np.array_equal(_host.check_noise_beta_args([0.9, 0.0], 2), f32([0.9, 0.0]))
    assert np.array_equal(_host.check_noise_beta_args(torch.tensor([0.25, 0.5]), 2), f32([0.25, 0.5]))
    assert np.array_equal(_host.check_noise_beta_args(np.array([0.999]), 1), f32([0.999]))
    assert _host.check_noise_beta_args(0.9, 2).dtype == np.float32
    for bad in (1.0, -0.1, 1.5, float("nan"), [0.5, 1.0], [0.5, -1e-3], [0.5], [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError):
            _host.check_noise_beta_args(bad, 2)
    with pytest.raises(ValueError, match="torch_cpu"):
        _host.check_noise_beta_args(0.5, 2, noise_source="torch_cpu")
    with pytest.raises(ValueError, match="action_cost"):
        _host.check_noise_beta_args([0.0, 0.5], 2, action_cost=True)
    # the two exclusions only bind when the filter is asked for
    _host.check_noise_beta_args(0.0, 2, noise_source="torch_cpu", action_cost=True)
    _host.check_noise_beta_args([0.0, 0.0], 2, noise_source="torch_cpu", action_cost=True)
