"""The reference of tests/test_gpu_noise_domain.py on its own (no GPU): tests/noise_ref.py reproduces the published
Philox4x32-10 known answers, its grids have the moments worked out for them, and the float32 rounding of the float64 factors —
the best any float32 implementation can do — satisfies every condition the GPU test puts on the device's tables.  The program
the GPU test runs cross-compiles here.
"""
import os
import subprocess

import numpy as np
import pytest

import noise_ref as nr
import test_gpu_noise_domain as dom
from mppi_playground_amd import _build


@pytest.mark.parametrize("counter, key, want", dom.KAT)
def test_philox_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds: zeros, all ones, and the digits of pi."""
    got = nr.philox4x32_10(*counter, *key)
    assert [int(w) for w in got] == list(want), [hex(int(w)) for w in got]


def test_philox_on_arrays_equals_philox_on_scalars():
    """The three vectors as one array call (ideal_normals calls it that way), with broadcast keys."""
    cols = [np.array([c[j] for c, _, _ in dom.KAT], np.uint64) for j in range(4)]
    for v, (_, key, want) in enumerate(dom.KAT):
        got = nr.philox4x32_10(*cols, *key)
        assert [int(w[v]) for w in got] == list(want)


def test_ideal_normals_layout():
    """Row i is global sample first + i (the high counter word moves at 2^32); columns 4r .. 4r + 3 are group r; a narrower
    R is a prefix; the solve index and both key words matter."""
    seed, first = dom.SEED, dom.FIRST
    z = nr.ideal_normals(seed, 3, first, 130, 5)
    assert z.shape == (130, 20) and z.dtype == np.float64 and np.isfinite(z).all()
    assert np.array_equal(nr.ideal_normals(seed, 3, first, 130, 2), z[:, :8])
    assert np.array_equal(nr.ideal_normals(seed, 3, first + 64, 66, 5), z[64:])
    x, y, zz, w = (int(v) for v in nr.philox4x32_10(1, 1, 2, 3, seed & 0xffffffff, seed >> 32))   # sample 2^32 + 1 = first + 67
    a, b = nr.box_muller64(x, y)
    c, d = nr.box_muller64(zz, w)
    assert z[67, 8:12].tolist() == [float(a), float(b), float(c), float(d)]
    for other in (nr.ideal_normals(seed, 4, first, 130, 5), nr.ideal_normals(seed ^ 1, 3, first, 130, 5),
                  nr.ideal_normals(seed ^ (1 << 32), 3, first, 130, 5), nr.ideal_normals(seed, 3, first + (1 << 32), 130, 5)):
        assert np.abs(other - z).max(axis=1).min() > 0.1   # every row is another draw


def test_ideal_moments():
    """What the grids themselves cost against N(0, 1), so that the GPU test is not charged for it: u1 never reaches 0 (the tail
    ends at 5.768) and is a right-endpoint rule for the integrals of -2 ln u and its square; the trig grid is exact."""
    ref = dom.reference()
    m = ref["m"]
    assert abs(m["Er2"] - 1.99999889890) < 1e-9 and abs(m["Er4"] - 7.99995924213) < 1e-9
    assert abs(m["rad_max"] - 5.76810754640) < 1e-9 and abs(dom.RAD_MAX - m["rad_max"]) < 1e-9 and m["rad_max"] < dom.Z_MAX
    assert ref["rad"][-1] == 0.0 and ref["rad"][0] == m["rad_max"]
    for key, want in (("Ec2", 0.5), ("Es2", 0.5), ("Ec4", 0.375), ("Es4", 0.375), ("Ec", 0.0), ("Es", 0.0), ("Ecs", 0.0)):
        assert abs(m[key] - want) < 1e-15, (key, m[key])
    assert abs(m["var"] - 0.99999944945) < 1e-9 and abs(m["var_s"] - 0.99999944945) < 1e-9
    assert abs(m["kurt"] - 2.99998801909) < 1e-9 and abs(m["kurt_s"] - 2.99998801909) < 1e-9
    c, s = ref["c"], ref["s"]
    assert [c[q] for q in dom.QUARTER_TURNS] == [1.0, 0.0, -1.0, 0.0] and [s[q] for q in dom.QUARTER_TURNS] == [0.0, 1.0, 0.0, -1.0]
    assert np.abs(c * c + s * s - 1.0).max() < 4e-16


def test_octaves_partition_the_radius_domain():
    u1 = nr.ideal_u1()
    e = np.floor(-np.log2(u1)).astype(np.int64)
    assert e.min() == 0 and e.max() == 24
    stop = nr.N_RADIUS
    for k in range(dom.OCTAVES):
        sl = dom.octave_slice(k)
        assert sl.stop == stop and (e[sl] == k).all()
        stop = sl.start
    assert stop == 0


def test_the_conditions_hold_for_the_rounded_reference():
    """float32(radius_64) and float32(trig_64): the radius is off by at most 2^-24 * 5.77 (half an ulp of at most 5.77), the
    trig values by at most 2^-25; ranges, ceiling, tripwires and moment bounds all hold for them."""
    ref = dom.reference()
    rad, c, s = ref["rad"].astype(np.float32), ref["c"].astype(np.float32), ref["s"].astype(np.float32)
    meas = dom.measure(rad, c, s)
    dom.report(meas, "rounded reference")
    assert meas["dr"] <= 2.0 ** -24 * 5.77 and meas["dt"] <= 2.0 ** -25 and meas["dt_quarter"] == 0.0
    assert max(meas["rel"]) <= 2.0 ** -24
    dom.check_ranges(rad, c, s)
    dom.check_ceiling(meas)
    dom.check_tripwires(meas)
    dom.check_moments(rad, c, s, "rounded reference")


def test_the_conditions_catch_wrong_tables():
    """Tables that are subtly wrong, made from the rounded reference: each is caught, and the small ones by the tripwires
    alone — the 1e-4 ceiling passes them, which is why the tripwires exist."""
    ref = dom.reference()
    rad, c, s = ref["rad"].astype(np.float32), ref["c"].astype(np.float32), ref["s"].astype(np.float32)

    def caught(check, *a):
        with pytest.raises(AssertionError):
            check(*a)

    # the angle one grid step off (b >> 9 read as b >> 9 plus one): 2 pi 2^-23 = 7.5e-7
    m = dom.measure(rad, np.roll(c, -1), np.roll(s, -1))
    dom.check_ceiling(m)
    caught(dom.check_tripwires, m)
    # the radius 3e-7 short, relative (the constant -2 ln 2 wrong in its seventh digit)
    short = (rad.astype(np.float64) * (1 - 3e-7)).astype(np.float32)
    m = dom.measure(short, c, s)
    dom.check_ceiling(m)
    caught(dom.check_tripwires, m)
    # u1 = n 2^-24 instead of (n + 1) 2^-24 (n = 0 would be u1 = 0: infinite), cos and sin exchanged, a negated sine: the
    # ceiling itself
    caught(dom.check_ranges, np.concatenate([np.float32([np.inf]), rad[:-1]]), c, s)
    caught(dom.check_ceiling, dom.measure(np.concatenate([rad[:1], rad[:-1]]), c, s))
    caught(dom.check_ceiling, dom.measure(rad, s, c))
    caught(dom.check_ceiling, dom.measure(rad, c, -s))
    # a radius that does not reach zero at u1 = 1, and one that dips below it
    caught(dom.check_ranges, np.concatenate([rad[:-1], np.float32([1e-6])]), c, s)
    caught(dom.check_ranges, np.concatenate([rad[:-2], np.float32([-1e-6, 0.0])]), c, s)


def test_moment_bounds_are_not_vacuous():
    """With no error allowed the bounds are zero, and they grow with either limit."""
    zero = dom.moment_bounds([0.0] * dom.OCTAVES, 0.0)
    assert all(abs(v) < 1e-15 for v in zero.values()), zero
    small, large = dom.moment_bounds([1e-6] * dom.OCTAVES, 1e-7), dom.moment_bounds([2e-6] * dom.OCTAVES, 2e-7)
    assert all(0 < small[k] < large[k] for k in small)
    # one dr for every octave: the plain statement (2 E[r] dr + dr^2) / 2 + E[r^2] (2 dt + dt^2) + 2^-23 covers it
    m = dom.reference()["m"]
    dr, dt = 1e-4, 1e-4 / dom.Z_MAX
    plain = (2 * m["Er"] * dr + dr ** 2) / 2 + m["Er2"] * (2 * dt + dt ** 2) + 2.0 ** -23
    assert dom.moment_bounds([dr] * dom.OCTAVES, dt)["var"] <= plain


def test_the_device_program_builds(tmp_path):
    try:
        hipcc = _build.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    flags = [f for f in _build.FLAGS if f not in ("-shared", "-fPIC")]
    exe = str(tmp_path / "noise_domain")
    subprocess.check_call([hipcc, *flags, "-I", _build.CSRC, dom.SRC, "-o", exe])
    assert os.path.getsize(exe) > 0
