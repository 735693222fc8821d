"""The plain reference of the device noise source (csrc/philox.hpp, gen_noise4 in csrc/mppi_sample.hpp): numpy only.

* philox4x32_10: Philox4x32 with ten rounds as Random123 defines it (Salmon, Moraes, Dror, Shaw, SC'11), on uint64 arrays, so
  every product and sum is an exact integer; held to the published known answers by tests/test_noise_ref_host.py.
* ideal_normals: that generator under the library's counter / key layout, followed by Box-Muller in float64.
* ideal_radius / ideal_trig: the two factors of a normal over EVERY operand that can reach them, float64.  box_muller is the
  product of a function of a >> 8 (2^24 values) and a function of b >> 9 (2^23 values), so the two tables are the whole domain.
* discrete_moments: the moments of the product distribution of two such tables (the ideal ones, or the device's).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57   # the round multipliers (of counter words 0 and 2)
W0, W1 = 0x9E3779B9, 0xBB67AE85   # the key schedule (Weyl) increments of key words 0 and 1
N_RADIUS, N_ANGLE = 1 << 24, 1 << 23
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10):
    """The four output words (uint64 arrays holding 32-bit values) of counter (c0, c1, c2, c3) under key (k0, k1)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(v, np.uint64) & _LOW for v in (c0, c1, c2, c3, k0, k1)])
    for r in range(rounds):
        if r:  # the key is bumped between rounds, not before the first
            k0, k1 = (k0 + np.uint64(W0)) & _LOW, (k1 + np.uint64(W1)) & _LOW
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2   # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LOW, (p0 >> _32) ^ c3 ^ k1, p0 & _LOW
    return c0, c1, c2, c3


def box_muller64(a, b):
    """float64 Box-Muller of the word pair (a, b): u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 9) 2^-23 in [0, 1)."""
    u1 = ((np.asarray(a, np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    c, s = _cos_sin_turns(np.asarray(b, np.uint64) >> np.uint64(9))
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * c, rad * s


def ideal_normals(seed, solve_idx, first, n, R):
    """float64 [n, 4R]: row i holds the 4R standard normals of global sample first + i at solve `solve_idx` — counter
    (gi lo, gi hi, r, solve_idx), key (seed lo, seed hi); normals 0, 1 of group r from words (x, y), normals 2, 3 from (z, w)."""
    gi = (np.uint64(first) + np.arange(n, dtype=np.uint64))[:, None]
    r = np.arange(R, dtype=np.uint64)[None, :]
    x, y, z, w = philox4x32_10(gi & _LOW, gi >> _32, r, solve_idx, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty((n, R, 4), np.float64)
    out[:, :, 0], out[:, :, 1] = box_muller64(x, y)
    out[:, :, 2], out[:, :, 3] = box_muller64(z, w)
    return out.reshape(n, 4 * R)


def ideal_u1():
    """u1 of every a >> 8, exact in float64: 2^-24 .. 1."""
    return (np.arange(N_RADIUS, dtype=np.float64) + 1.0) * 2.0 ** -24


def ideal_radius():
    """sqrt(-2 ln u1) for every a >> 8 (index n: u1 = (n + 1) 2^-24): 5.768 .. 0."""
    return np.sqrt(-2.0 * np.log(ideal_u1()))


def _cos_sin_turns(m):
    """(cos, sin)(2 pi m 2^-23), m < 2^23 an integer array.  The quarter turn is taken off exactly in integers, so the
    argument of libm lies in [0, pi/2) and the values AT the quarter turns are exactly 0 and +-1."""
    m = np.asarray(m, np.uint64)
    q = (m >> np.uint64(21)).astype(np.int64)
    phi = (m & np.uint64((1 << 21) - 1)).astype(np.float64) * (2.0 * np.pi * 2.0 ** -23)
    c0, s0 = np.cos(phi), np.sin(phi)
    c = np.choose(q, [c0, -s0, -c0, s0])
    s = np.choose(q, [s0, c0, -s0, -c0])
    return c + 0.0, s + 0.0   # (-0 -> +0)


def ideal_trig():
    """(cos, sin)(2 pi u2) for every b >> 9 (index m: u2 = m 2^-23)."""
    return _cos_sin_turns(np.arange(N_ANGLE, dtype=np.uint64))


def discrete_moments(rad, c, s):
    """Moments of z0 = rad * c and z1 = rad * s with the index of `rad` and the index of (c, s) independent and uniform —
    what the generator's words are.  The factors separate, so 2^24 + 2^23 values give the moments over all 2^47 pairs."""
    rad, c, s = (np.asarray(v, np.float64) for v in (rad, c, s))
    r2 = rad * rad
    c2, s2 = c * c, s * s
    Er2, Er4 = r2.mean(), (r2 * r2).mean()
    Ec2, Es2, Ec4, Es4 = c2.mean(), s2.mean(), (c2 * c2).mean(), (s2 * s2).mean()
    var, var_s = Er2 * Ec2, Er2 * Es2
    return dict(Er=rad.mean(), Er2=Er2, Er4=Er4, Ec2=Ec2, Es2=Es2, Ec4=Ec4, Es4=Es4, var=var, var_s=var_s,
                kurt=Er4 * Ec4 / var ** 2, kurt_s=Er4 * Es4 / var_s ** 2, Ec=c.mean(), Es=s.mean(), Ecs=(c * s).mean(),
                rad_max=rad.max())
