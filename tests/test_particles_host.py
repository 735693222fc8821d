"""Risk-aware solves without a GPU: the numpy restatement of the particle fold (pi_mpc._host.fold_particle_costs, the
operation order of include/mppi_hip.h) against a float64 evaluation, its edge cases, risk_alpha -> k, and the argument errors
of the constructor and the setters (raised before a device handle is touched).

k = P under CVaR is the DESCENDING-ORDER mean: the same addends as MEAN in another order, so the two agree to the bound of a
sequential fp32 sum and need not agree to the bit (test_cvar_edges shows a matrix where they differ)."""
import numpy as np
import pytest
import torch

import particle_cases as pc
from pi_mpc import _host

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("P", pc.SIZES_P)
def test_fold_against_float64(kind, P):
    m = pc.matrix(kind, P, 300)
    for mode in pc.MODES:
        for k in (pc.ks(P) if mode == "cvar" else (1,)):
            got = _host.fold_particle_costs(m, mode, k)
            assert got.dtype == f32 and got.shape == (300,)
            want, lim = pc.fold64(m, mode, k), pc.bound64(m, mode, k)
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= lim + 2.0 ** -24 * np.abs(want)), (kind, P, mode, k, float((err - lim).max()))
            if mode == "worst":
                assert np.array_equal(bits(got), bits(m.max(0)))


def test_operation_order_is_the_headers():
    """Sequential from c[0] (MEAN) / from the largest (CVaR), one rounding per operation: values whose sum depends on the order."""
    m = f32([[1.0e8], [1.0], [-1.0e8], [1.0]])
    a = f32(f32(f32(f32(1.0e8) + f32(1.0)) + f32(-1.0e8)) + f32(1.0)) / f32(4)
    assert np.array_equal(bits(_host.fold_particle_costs(m, "mean")), bits([a]))
    c = f32(f32(f32(f32(1.0e8) + f32(1.0)) + f32(1.0)) + f32(-1.0e8)) / f32(4)  # descending: 1e8, 1, 1, -1e8
    assert np.array_equal(bits(_host.fold_particle_costs(m, "cvar", 4)), bits([c]))
    assert _host.fold_particle_costs(m, 0)[0] == a and _host.fold_particle_costs(m, 2, 4)[0] == c  # (MPPI_RISK_* ids)


def test_cvar_edges():
    for kind in pc.KINDS:
        for P in pc.SIZES_P:
            m = pc.matrix(kind, P, 65, seed=1)
            worst = _host.fold_particle_costs(m, "worst")
            assert np.array_equal(bits(_host.fold_particle_costs(m, "cvar", 1)), bits(worst)), (kind, P)  # k = 1 IS the worst case
            full = _host.fold_particle_costs(m, "cvar", P)
            s = -np.sort(-m, axis=0)  # k = P: the descending-order mean ...
            assert np.array_equal(bits(full), bits(_host.fold_particle_costs(s, "mean"))), (kind, P)
            for k in range(1, P):  # the mean of the k worst does not grow with k
                a, b = _host.fold_particle_costs(m, "cvar", k), _host.fold_particle_costs(m, "cvar", k + 1)
                slack = pc.bound64(m, "cvar", k) + pc.bound64(m, "cvar", k + 1) + np.spacing(np.maximum(np.abs(a), np.abs(b)))
                assert np.all(b <= a + slack), (kind, P, k)  # (exact in float64; each side carries its sum's roundings)
    # ... which need not equal MEAN to the bit: the same addends in another order
    m = f32([[1.0e8], [-1.0e8], [1.0], [1.0]])  # MEAN: ((0 + 1) + 1) / 4 = 0.5; descending: ((1e8 + 1) + 1) - 1e8 = 0
    assert _host.fold_particle_costs(m, "cvar", 4)[0] != _host.fold_particle_costs(m, "mean")[0]


def test_single_particle_and_ties_and_negative():
    m = pc.matrix("magnitudes", 1, 300)
    for mode in pc.MODES:
        assert np.array_equal(bits(_host.fold_particle_costs(m, mode, 1)), bits(m[0])), mode  # x / 1.0f
    t = np.full((5, 7), f32(-3.25))
    for mode in pc.MODES:
        for k in (1, 2, 5):
            assert np.array_equal(bits(_host.fold_particle_costs(t, mode, k)), bits(t[0])), (mode, k)  # -3.25 * n / n is exact
    n = f32([[-1.0, -8.0], [-2.0, -4.0], [-4.0, -2.0]])
    assert np.array_equal(_host.fold_particle_costs(n, "worst"), f32([-1.0, -2.0]))
    assert np.array_equal(_host.fold_particle_costs(n, "cvar", 2), f32([-1.5, -3.0]))


def test_nan_makes_the_folded_cost_nan():
    m = pc.matrix("mixed", 3, 8)
    m[1, 2] = np.nan
    for mode in pc.MODES:
        out = _host.fold_particle_costs(m, mode, 2)
        assert np.isnan(out[2]) and np.all(np.isfinite(np.delete(out, 2))), mode


def test_fold_argument_errors():
    m = pc.matrix("mixed", 3, 8)
    for k in (0, 4):
        with pytest.raises(ValueError):
            _host.fold_particle_costs(m, "cvar", k)
    with pytest.raises(ValueError):
        _host.fold_particle_costs(m, "median")
    with pytest.raises(ValueError):
        _host.fold_particle_costs(m[0], "mean")


def test_risk_alpha_to_k():
    assert [_host.risk_k(1.0, P) for P in (1, 2, 8, 16)] == [1, 2, 8, 16]
    assert [_host.risk_k(1e-9, P) for P in (1, 2, 8, 16)] == [1, 1, 1, 1]       # never below one particle
    assert _host.risk_k(0.25, 8) == 2 and _host.risk_k(0.25, 5) == 2 and _host.risk_k(0.2, 5) == 1
    assert _host.risk_k(0.125, 16) == 2 and _host.risk_k(0.126, 16) == 3          # the ceiling
    assert _host.risk_k(0.5, 3) == 2 and _host.risk_k(1.0 / 3.0, 3) == 1
    assert _host.risk_k(0.9999999, 16) == 16 and _host.risk_k(0.5, 1) == 1        # never above P


def test_risk_argument_errors():
    assert _host.check_risk_args("cvar", 0.25) == ("cvar", 0.25) and _host.check_risk_args("mean", 1) == ("mean", 1.0)
    for bad in ("median", None, 2):
        with pytest.raises(ValueError):
            _host.check_risk_args(bad, 1.0)
    for bad in (0.0, -0.1, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _host.check_risk_args("cvar", bad)


def test_particle_shape_errors():
    assert _host.check_particles_shape((3, 4), 4) == 3 and _host.check_particles_shape(torch.zeros(16, 2).shape, 2) == 16
    for shape in ((17, 4), (0, 4), (3, 5), (4,), (1, 3, 4)):
        with pytest.raises(ValueError):
            _host.check_particles_shape(shape, 4)


def _ctor_kwargs(**kw):
    from envs.classic_control import pendulum_cost, pendulum_dynamics

    return dict(horizon=5, num_samples=64, dim_state=2, dim_control=1, dynamics=pendulum_dynamics, cost_func=pendulum_cost,
                u_min=torch.tensor([-2.0]), u_max=torch.tensor([2.0]), sigmas=torch.tensor([1.0]), lambda_=1.0, **kw)


@pytest.mark.parametrize("kw", [dict(risk="median"), dict(risk="cvar", risk_alpha=0.0), dict(risk="cvar", risk_alpha=1.5),
                                dict(risk="worst", risk_alpha=-1.0)])
def test_constructor_refuses_before_the_device(kw):
    """ValueError with or without a GPU: the risk arguments are checked before the device and the handle are."""
    from pi_mpc.mppi import MPPI

    with pytest.raises(ValueError, match="risk"):
        MPPI(**_ctor_kwargs(**kw))


def test_setters_refuse_before_the_handle():
    """set_state_particles / set_risk on an object without a handle: the argument errors come first."""
    from pi_mpc.mppi import MPPI

    s = MPPI.__new__(MPPI)
    s.__dict__.update(_dim_state=4, _risk="mean", _risk_alpha=1.0, _particles_P=0, _particles_keep=None, _h=None, _ctor={})
    for t in (torch.zeros(17, 4), torch.zeros(3, 5), torch.zeros(4), np.zeros((0, 4), f32)):
        with pytest.raises(ValueError, match="state particles"):
            s.set_state_particles(t)
    for args in (("median",), ("cvar", 0.0), ("cvar", 2.0)):
        with pytest.raises(ValueError, match="risk"):
            s.set_risk(*args)
    assert s.risk == ("mean", 1.0)  # (a refused setting changes nothing)
    s.set_state_particles(None)     # off while off: no call into the library
