"""The control-cost term (action_cost=True, src/pi_mpc/mppi.py:294-316,330-336), the parts that need no GPU: the scalar pieces of
csrc/mppi_action_cost.hpp (the text the device kernels compile, built here with g++) against the numpy fp32 restatement of
tests/action_cost_ref.py bit for bit and against float64 within its first-order bound, the validation of the MPPI keyword
arguments, and one run of a stand-alone program around the header under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import action_cost_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mppi_playground_amd", "csrc", "mppi_action_cost.hpp")
f32 = np.float32

# costs[i] = c0[i] + kappa * A_i over rows [N][T][dc], through the header's pieces in the kernels' order
WALK = r"""
#include "%s"
extern "C" void g_table(const float* mean, const float* s, int T, int dc, float* inv, float* g) {
    for (int f = 0; f < T * dc; ++f) {
        inv[f] = mppi::action_cost_inv(f / dc, s[f]);
        g[f] = mppi::action_cost_g(mean[f], inv[f]);
    }
}
extern "C" void term(const float* g, const float* U, const float* c0, long N, int row, float weight, float lambda,
                     float* A_out, float* cost) {
    const float kappa = mppi::action_cost_kappa(weight, lambda);
    for (long i = 0; i < N; ++i) {
        float A = 0.0f;
        for (int f = 0; f < row; ++f) A = mppi::action_cost_accumulate(A, g[f], U[i * row + f]);
        A_out[i] = A;
        cost[i] = mppi::action_cost_total(c0[i], kappa, A);
    }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("action_cost")
    src = d / "walk.cpp"
    src.write_text(WALK % HEADER)
    so = d / "libwalk.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.g_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.g_table.restype = None
    lib.term.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    lib.term.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(lib, mean, s, U, c0, weight, lam):
    T, dc = mean.shape
    mean, s, U, c0 = (np.ascontiguousarray(a, f32) for a in (mean, np.broadcast_to(s, mean.shape), U, c0))
    inv, g = np.empty((T, dc), f32), np.empty((T, dc), f32)
    lib.g_table(_p(mean), _p(s), T, dc, _p(inv), _p(g))
    A, cost = np.empty(len(U), f32), np.empty(len(U), f32)
    lib.term(_p(g), _p(U), _p(c0), len(U), T * dc, weight, lam, _p(A), _p(cost))
    return inv, g, A, cost


def _case(rng, T, dc, saturated=False, zero_mean=False):
    N = 257
    lo, hi = -rng.uniform(0.5, 3.0, dc).astype(f32), rng.uniform(0.5, 3.0, dc).astype(f32)
    s = rng.uniform(0.05, 2.0, dc).astype(f32)
    mean = np.zeros((T, dc), f32) if zero_mean else rng.uniform(lo, hi, (T, dc)).astype(f32)
    scale = 3.0 * (hi - lo) if saturated else s
    U = np.clip(mean[None] + (rng.standard_normal((N, T, dc)) * scale).astype(f32), lo, hi).astype(f32)
    c0 = (rng.standard_normal(N) * 50.0 + 100.0).astype(f32)
    return mean, s, U, c0, lo, hi


@pytest.mark.parametrize("dc", [1, 2, 3, 6])
@pytest.mark.parametrize("T", [1, 2, 5, 16])
def test_pieces_equal_the_numpy_statement(lib, T, dc):
    rng = np.random.default_rng(100 * T + dc)
    for saturated, zero_mean, weight, lam in ((False, False, 1.0, 0.7), (True, False, 1.0, 20.0), (False, False, 0.0, 3.0),
                                              (False, True, 1.0, 3.0), (False, False, 0.37, 1.3)):
        mean, s, U, c0, lo, hi = _case(rng, T, dc, saturated, zero_mean)
        if saturated:
            assert np.mean((U == lo) | (U == hi)) > 0.5
        inv, g, A, cost = run(lib, mean, s, U, c0, weight, lam)
        want_g = ref.g32(mean, s)
        assert np.array_equal(inv[0], np.zeros(dc, f32))  # row 0 of the inverse covariance stays zero
        assert np.array_equal(inv[1:], np.broadcast_to((f32(1.0) / (s * s).astype(f32)).astype(f32), (T - 1, dc)))
        assert np.array_equal(g.view(np.uint32), want_g.view(np.uint32))
        assert np.array_equal(A.view(np.uint32), ref.A32(want_g, U).view(np.uint32))
        kappa = ref.kappa32(weight, lam)
        ref.check(f"T{T}_dc{dc}_sat{int(saturated)}_w{weight}", cost, c0, kappa, want_g, U)
        if weight == 0.0 or zero_mean or T == 1:
            assert np.array_equal(cost.view(np.uint32), c0.view(np.uint32))


def test_row_zero_contributes_exactly_nothing(lib):
    """Changing mean[0] and U[:, 0] changes no bit of A or of the cost."""
    rng = np.random.default_rng(7)
    mean, s, U, c0, lo, hi = _case(rng, 5, 2)
    _, _, A, cost = run(lib, mean, s, U, c0, 1.0, 2.0)
    mean2, U2 = mean.copy(), U.copy()
    mean2[0] = hi
    U2[:, 0] = rng.uniform(lo, hi, (len(U), 2)).astype(f32)
    _, g2, A2, cost2 = run(lib, mean2, s, U2, c0, 1.0, 2.0)
    assert np.array_equal(g2[0], np.zeros(2, f32))
    assert np.array_equal(A.view(np.uint32), A2.view(np.uint32)) and np.array_equal(cost.view(np.uint32), cost2.view(np.uint32))
    assert np.any(A != 0.0)


def test_per_step_sigma_table(lib):
    """s as a [T, dc] table (adapt_covariance): g follows the table's own row."""
    rng = np.random.default_rng(11)
    mean, _, U, c0, _, _ = _case(rng, 16, 2)
    s = rng.uniform(0.05, 1.5, (16, 2)).astype(f32)
    _, g, A, cost = run(lib, mean, s, U, c0, 1.0, 5.0)
    assert np.array_equal(g.view(np.uint32), ref.g32(mean, s).view(np.uint32))
    ref.check("table", cost, c0, ref.kappa32(1.0, 5.0), ref.g32(mean, s), U)


def test_keyword_validation():
    from pi_mpc import _host  # (tests/conftest.py imports mppi_playground_amd, which puts pi_mpc/ on the path)

    sig = np.array([0.5, 1.0], f32)
    assert _host.check_action_cost_args(True, 1.0, sig) == 1.0
    assert _host.check_action_cost_args(True, 0.0, sig) == 0.0
    assert _host.check_action_cost_args(False, 0.25, np.array([0.0, 1.0], f32)) == 0.25  # sigmas only bind with the term on
    for w in (-0.1, float("nan"), float("inf")):
        for on in (True, False):
            with pytest.raises(ValueError):
                _host.check_action_cost_args(on, w, sig)
    for bad in ([0.0, 1.0], [-0.5, 1.0]):
        with pytest.raises(ValueError, match="sigmas"):
            _host.check_action_cost_args(True, 1.0, np.array(bad, f32))
    # the adapted table must not be able to reach zero
    with pytest.raises(ValueError, match="cov_floor"):
        _host.check_action_cost_args(True, 1.0, sig, adapt_covariance=True, cov_floor=0.0)
    with pytest.raises(ValueError, match="cov_floor"):
        _host.check_action_cost_args(True, 1.0, sig, adapt_covariance=True, cov_floor=0.0, sigma_min=np.array([0.1, 0.0], f32))
    _host.check_action_cost_args(True, 1.0, sig, adapt_covariance=True, cov_floor=0.0, sigma_min=np.array([0.1, 0.05], f32))
    _host.check_action_cost_args(True, 1.0, sig, adapt_covariance=True, cov_floor=1e-6)
    _host.check_action_cost_args(True, 1.0, sig, adapt_covariance=False, cov_floor=0.0)


MAIN = r"""
#include <cstdio>
#include <vector>
#include "%s"
int main() {
    const int T = 16, dc = 3, N = 65;
    std::vector<float> mean(T * dc), s(T * dc), g(T * dc), U((size_t)N * T * dc), cost(N);
    for (int f = 0; f < T * dc; ++f) { mean[f] = 0.01f * (f %% 7) - 0.02f; s[f] = 0.1f + 0.05f * (f %% 5); }
    for (size_t j = 0; j < U.size(); ++j) U[j] = 0.001f * (float)(j %% 977) - 0.4f;
    for (int f = 0; f < T * dc; ++f) g[f] = mppi::action_cost_g(mean[f], mppi::action_cost_inv(f / dc, s[f]));
    const float kappa = mppi::action_cost_kappa(1.0f, 2.5f);
    double sum = 0.0;
    for (int i = 0; i < N; ++i) {
        float A = 0.0f;
        for (int f = 0; f < T * dc; ++f) A = mppi::action_cost_accumulate(A, g[f], U[(size_t)i * T * dc + f]);
        cost[i] = mppi::action_cost_total(3.0f, kappa, A);
        sum += cost[i];
    }
    for (int k = 0; k < dc; ++k) if (g[k] != 0.0f) return 2;
    std::printf("%%.9g\n", sum);
    return 0;
}
"""


def test_standalone_program_under_sanitizers(tmp_path):
    """The header inside a program of its own (its own main), built with -fsanitize=address,undefined and run once."""
    src = tmp_path / "main.cpp"
    src.write_text(MAIN % HEADER)
    exe = tmp_path / "action_cost_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert np.isfinite(float(out.stdout))
