"""The control-cost term (src/pi_mpc/mppi.py:294-316,330-336) restated in numpy, shared by the CPU and the GPU tests:
the fp32 statement the device is held to bit for bit, and the float64 value with the first-order error bound of that fp32
statement."""
import numpy as np

f32 = np.float32


def g32(mean, s):
    """g[T,dc] = fl32(mean * inv), inv = 0 for t = 0 and fl32(1 / fl32(s * s)) for t >= 1 (s[T,dc] or [dc])."""
    mean = np.asarray(mean, f32)
    s = np.broadcast_to(np.asarray(s, f32), mean.shape)
    with np.errstate(divide="ignore"):
        inv = (f32(1.0) / (s * s).astype(f32)).astype(f32)
    inv = inv.copy()
    inv[0] = 0.0
    return (mean * inv).astype(f32)


def A32(g, U):
    """A[N]: sequential fp32 sum over t, then k, of fl32(g[t,k] * U[i,t,k]) — separate multiply and add."""
    g, U = np.asarray(g, f32), np.asarray(U, f32)
    N = U.shape[0]
    gf, Uf = g.reshape(-1), U.reshape(N, -1)
    A = np.zeros(N, f32)
    for j in range(gf.shape[0]):
        A = (A + (gf[j] * Uf[:, j]).astype(f32)).astype(f32)
    return A


def kappa32(weight, lam):
    return f32(f32(weight) * f32(lam))


def total32(c0, kappa, A):
    """cost = fl32(c0 + fl32(kappa * A))"""
    return (np.asarray(c0, f32) + (f32(kappa) * np.asarray(A, f32)).astype(f32)).astype(f32)


def A64(g, U):
    """(A in float64 from the fp32 g and U, sum |g * U|)"""
    g, U = np.asarray(g, np.float64), np.asarray(U, np.float64)
    p = g[None] * U
    return p.reshape(len(U), -1).sum(1), np.abs(p).reshape(len(U), -1).sum(1)


def check(name, c1, c0, kappa, g, U):
    """(a) c1 == fl32(c0 + fl32(kappa * A32)) bit for bit and (b) |c1 - (c0 + kappa * A64)| <= 2 * 2^-24 * (|c1| + (T * dc + 1) *
    kappa * sum |g * U|) for EVERY sample: the first-order bound of a sequential fp32 sum of T * dc products plus two roundings,
    doubled."""
    c1, c0 = np.asarray(c1, f32), np.asarray(c0, f32)
    assert c1.shape == c0.shape == (len(U),)
    want = total32(c0, kappa, A32(g, U))
    bad = np.flatnonzero(want.view(np.uint32) != c1.view(np.uint32))
    a64, absum = A64(g, U)
    n = g.size
    k = float(kappa)
    err = np.abs(c1.astype(np.float64) - (c0.astype(np.float64) + k * a64))
    bound = 2.0 * 2.0 ** -24 * (np.abs(c1.astype(np.float64)) + (n + 1) * k * absum)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if len(err) else 0.0
    print(f"[action_cost] {name}: N {len(U)}, kappa {k:.6g}, bit mismatches {len(bad)}, worst err / bound {ratio:.3f}, "
          f"max |kappa A| {float(np.max(np.abs(k * a64))):.4g}")
    assert len(bad) == 0, f"{name}: {len(bad)} samples differ from the fp32 statement, first {bad[:5]}: {c1[bad[:5]]} vs {want[bad[:5]]}"
    assert np.all(err <= bound), f"{name}: float64 bound missed, worst err / bound {ratio:.3f}"
