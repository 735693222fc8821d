"""The normal draw (csrc/philox.hpp: philox4x32_10, box_muller) against float64 over EVERY input, and Philox against the
published known answers — on a real MI355X.

box_muller(a, b) is radius(a >> 8) * (cos, sin)(b >> 9): a function of 2^24 values times a function of 2^23 values.  A small
program (tests/gpu_progs/noise_domain.hip, built here with the library's own flags) evaluates both factors on the device for
every operand and writes the tables; the float64 reference is numpy's (tests/noise_ref.py).  With

    dr = max |radius_dev - radius_64|     dt = max |trig_dev - trig_64| (both tables)

every one of the 2^47 products obeys  |fl(r' c') - r c| <= |r' - r| |c'| + r |c' - c| + |r' c'| 2^-24
                                                        <= dr (1 + dt) + 5.7682 dt + 5.7682 2^-24
(r <= 5.76810754640, |c| <= 1; dr dt is below 2e-9 under the ceiling and is carried by the margin of 5.7682 over the largest
radius times (1 + dt)).  The program also multiplies the two tables on the device and holds both instantiations of box_muller
to those products bit for bit, so the tables measured here ARE the factors the library multiplies.

* exact conditions (derived): the 24 known-answer words; both overloads of philox4x32_10 equal; bm_u1_mul's radius equal to
  bm_u1_fma's; every value finite, the radius non-negative, zero at u1 = 1 and at most the ideal maximum plus the limit.
* the ceiling: CEILING = 1e-4 is what test_sampler_matches_philox_restatement states of 100 000 draws
  (|eps - ref| < 1e-4 sigma); here it holds on all 2^47 pairs: dr + 5.7682 dt + 5.7682 2^-24 <= 1e-4.
* tripwires: dr per octave e = floor(-log2 u1) of the radius operand, absolute and relative, and dt overall and at the four
  quarter turns, each at most 2 x the value recorded in profiles/noise_domain.md (and never more than the ceiling allows).
  2 x: the domain is exhaustive and the hardware functions are deterministic, so there is no run-to-run spread; the factor
  only absorbs another host libm under the float64 reference, and a factor computed with one bit less roughly doubles.
* moments of the device's own distribution (noise_ref.discrete_moments of the device tables) against the ideal grids', held to
  what the asserted pointwise limits imply (moment_bounds below) — no fitted number.
* the shipped library draws this stream: mppi_sample + mppi_export_noise and mppi_sample_posterior of generic handles equal
  the program's `stream` mode bit for bit, and lie within the pointwise limit of numpy Philox + float64 Box-Muller.

The conditions are functions of three float32 tables, so tests/test_noise_ref_host.py runs them on the float32 rounding of
the reference itself: they are satisfiable before any device value enters.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import noise_ref as nr
from mppi_playground_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gpu_progs", "noise_domain.hip")

CEILING = 1e-4            # tests/test_gpu_parity.py::test_sampler_matches_philox_restatement: |eps - ref| < 1e-4 * sigma
Z_MAX = 5.7682            # the ceiling's weight of dt and of the product's rounding: above the largest radius (1 + dt)
RAD_MAX = 5.76810754640   # sqrt(-2 ln 2^-24)
OCTAVES = 25              # e = floor(-log2 u1) = 0 .. 24
QUARTER_TURNS = (0, 1 << 21, 1 << 22, 3 << 21)

# Measured maxima on the MI355X: profiles/noise_domain.md (the per-octave table and the trig maxima, with date and ROCm
# version).  Index = octave e.  The tests allow 2 x each.
RADIUS_ABS = [1.246e-07, 1.438e-07, 2.532e-07, 2.449e-07, 2.886e-07, 2.648e-07, 2.848e-07, 2.833e-07, 3.612e-07,   # e = 0 .. 8
              3.539e-07, 3.250e-07, 4.878e-07, 4.387e-07, 3.918e-07, 4.010e-07, 4.143e-07, 4.140e-07, 3.609e-07,   # 9 .. 17
              4.105e-07, 2.037e-07, 3.618e-07, 2.028e-07, 3.873e-07, 2.508e-07, 1.322e-07]   # profiles/noise_domain.md, "abs"
RADIUS_REL = [1.370e-07, 1.174e-07, 1.249e-07, 1.175e-07, 1.220e-07, 9.921e-08, 9.443e-08, 8.608e-08, 1.041e-07,   # e = 0 .. 8
              1.000e-07, 8.631e-08, 1.202e-07, 1.060e-07, 8.916e-08, 8.977e-08, 8.999e-08, 8.641e-08, 7.370e-08,   # 9 .. 17
              8.090e-08, 3.955e-08, 6.800e-08, 3.759e-08, 6.947e-08, 4.441e-08, 2.291e-08]   # profiles/noise_domain.md, "rel"
#                                                                     (the point u1 = 1, radius 0, has no relative error)
TRIG_ABS = 1.253e-07          # profiles/noise_domain.md, "trig, every angle" (cos and sin alike)
TRIG_QUARTER_ABS = 0.0        # profiles/noise_domain.md, "trig, quarter turns": exactly 0 and +-1 there
MARGIN = 2.0


def octave_slice(e):
    """The indices n = a >> 8 whose u1 = (n + 1) 2^-24 lies in octave e: 2^-(e+1) < u1 <= 2^-e."""
    return slice(0 if e == 24 else 1 << (23 - e), 1 << (24 - e))


# ---------------------------------------------------------------------------------------------- limits (no device value)
def radius_abs_limit(e):
    return min(MARGIN * RADIUS_ABS[e], CEILING)


def radius_rel_limit(e):
    return MARGIN * RADIUS_REL[e]


def trig_limit():
    return min(MARGIN * TRIG_ABS, CEILING / Z_MAX)


def trig_quarter_limit():
    return min(MARGIN * TRIG_QUARTER_ABS, trig_limit())


def pointwise_limit():
    """What the asserted limits leave of |z_dev - z_64| for any pair: the ceiling's expression on the limits, at most the
    ceiling (which the measured dr and dt are held to directly)."""
    dr = max(radius_abs_limit(e) for e in range(OCTAVES))
    return min(dr + Z_MAX * trig_limit() + Z_MAX * 2.0 ** -24, CEILING)


@functools.lru_cache(maxsize=None)
def reference():
    """The float64 tables and what the bounds need of them; computed once per process."""
    rad = nr.ideal_radius()
    c, s = nr.ideal_trig()
    ref = dict(rad=rad, c=c, s=s, m=nr.discrete_moments(rad, c, s))
    # per octave: its probability and the conditional means of r, r^2, r^3
    ref["p"] = [(octave_slice(e).stop - octave_slice(e).start) / nr.N_RADIUS for e in range(OCTAVES)]
    ref["r1"], ref["r2"], ref["r3"] = ([float((rad[octave_slice(e)] ** k).mean()) for e in range(OCTAVES)] for k in (1, 2, 3))
    for v in (rad, c, s):
        v.setflags(write=False)
    return ref


def moment_bounds(dr, dt):
    """Bounds on |moment(device tables) - moment(ideal tables)| from pointwise limits alone: dr[e] on the radius in octave e,
    dt on both trig tables.  r' = r + d with |d| <= dr[e], c' = c + g with |g| <= dt, |c| <= 1; p_e, E[r^k | e] ideal.

      |E r'^2 - E r^2| <= sum_e p_e (2 E[r|e] dr_e + dr_e^2)                                   =: A2
      |E r'^4 - E r^4| <= sum_e p_e (4 E[r^3|e] dr_e + 6 E[r^2|e] dr_e^2 + 4 E[r|e] dr_e^3 + dr_e^4)   =: A4
      |E c'^2 - E c^2| <= 2 dt + dt^2 =: B2        |E c'^4 - E c^4| <= 4 dt + 6 dt^2 + 4 dt^3 + dt^4 =: B4
      var' - var = (E r'^2 - E r^2) E c'^2 + E r^2 (E c'^2 - E c^2):  |d var| <= A2 (E c^2 + B2) + E r^2 B2
        (with one dr for all octaves this is the (2 E[r] dr + dr^2) / 2 + E[r^2] (2 dt + dt^2) + A2 B2 of the plain statement,
        A2 B2 < 2^-23 under the ceiling)
      N = E r^4 E c^4:  |dN| <= A4 (E c^4 + B4) + E r^4 B4;  kurtosis' lies in [(N - dN) / (var + dvar)^2, (N + dN) / (var - dvar)^2]
      |E c' - E c| <= dt (and sin)       |E c's' - E cs| <= E |c'| |s' - s| + E |s| |c' - c| <= (1 + dt) dt + dt
    """
    ref = reference()
    m, p, r1, r2, r3 = ref["m"], ref["p"], ref["r1"], ref["r2"], ref["r3"]
    A2 = sum(p[e] * (2 * r1[e] * dr[e] + dr[e] ** 2) for e in range(OCTAVES))
    A4 = sum(p[e] * (4 * r3[e] * dr[e] + 6 * r2[e] * dr[e] ** 2 + 4 * r1[e] * dr[e] ** 3 + dr[e] ** 4) for e in range(OCTAVES))
    B2 = 2 * dt + dt ** 2
    B4 = 4 * dt + 6 * dt ** 2 + 4 * dt ** 3 + dt ** 4
    out = {}
    for var, c2, c4, kurt, tag in ((m["var"], m["Ec2"], m["Ec4"], m["kurt"], ""), (m["var_s"], m["Es2"], m["Es4"], m["kurt_s"], "_s")):
        dvar = A2 * (c2 + B2) + m["Er2"] * B2
        N = m["Er4"] * c4
        dN = A4 * (c4 + B4) + m["Er4"] * B4
        out["var" + tag] = dvar
        out["kurt" + tag] = max((N + dN) / (var - dvar) ** 2 - kurt, kurt - (N - dN) / (var + dvar) ** 2)
    out["Ec"] = out["Es"] = dt
    out["Ecs"] = (1 + dt) * dt + dt
    return out


# ------------------------------------------------------------------------------------- the conditions on three float32 tables
def measure(rad, c, s):
    """Errors of float32 tables against the float64 reference: per octave (absolute, relative, where), trig overall and at the
    quarter turns."""
    ref = reference()
    err = np.abs(rad.astype(np.float64) - ref["rad"])
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref["rad"] > 0, err / ref["rad"], 0.0)
    out = dict(abs=[], rel=[], abs_at=[], rel_at=[])
    for e in range(OCTAVES):
        sl = octave_slice(e)
        ia, ir = int(err[sl].argmax()), int(rel[sl].argmax())
        out["abs"].append(float(err[sl][ia])); out["abs_at"].append(sl.start + ia)
        out["rel"].append(float(rel[sl][ir])); out["rel_at"].append(sl.start + ir)
    ec, es = np.abs(c.astype(np.float64) - ref["c"]), np.abs(s.astype(np.float64) - ref["s"])
    out["cos"], out["cos_at"], out["sin"], out["sin_at"] = float(ec.max()), int(ec.argmax()), float(es.max()), int(es.argmax())
    out["dt"] = max(out["cos"], out["sin"])
    q = list(QUARTER_TURNS)
    out["dt_quarter"] = float(max(ec[q].max(), es[q].max()))
    out["dr"] = max(out["abs"])
    return out


def report(meas, who):
    for e in range(OCTAVES):
        print(f"[noise] {who} radius octave {e:2d}: largest so far {meas['abs'][e]:.3e} at n = {meas['abs_at'][e]}, "
              f"relative {meas['rel'][e]:.3e} at n = {meas['rel_at'][e]}")
    print(f"[noise] {who} trig: largest so far cos {meas['cos']:.3e} at m = {meas['cos_at']}, sin {meas['sin']:.3e} at m = "
          f"{meas['sin_at']}; at the quarter turns {meas['dt_quarter']:.3e}")
    print(f"[noise] {who} ceiling: dr {meas['dr']:.3e} + {Z_MAX} * dt {meas['dt']:.3e} + {Z_MAX} * 2^-24 = "
          f"{meas['dr'] + Z_MAX * meas['dt'] + Z_MAX * 2.0 ** -24:.3e} (<= {CEILING:g})")


def check_ranges(rad, c, s):
    assert rad.dtype == c.dtype == s.dtype == np.float32
    assert (rad.size, c.size, s.size) == (nr.N_RADIUS, nr.N_ANGLE, nr.N_ANGLE)
    assert np.isfinite(rad).all() and np.isfinite(c).all() and np.isfinite(s).all()
    assert rad[-1] == 0.0, f"radius(u1 = 1) = {rad[-1]!r}"        # (either sign)
    assert not (rad < 0).any(), f"negative radius at n = {int(np.argmax(rad < 0))}"
    top = RAD_MAX + radius_abs_limit(24)   # (the largest radius is octave 24's single point; every limit is <= the ceiling)
    assert rad.max() <= top, f"radius {rad.max()!r} at n = {int(rad.argmax())} above {top!r}"
    lim = 1.0 + trig_limit()
    assert np.abs(c).max() <= lim and np.abs(s).max() <= lim, (float(np.abs(c).max()), float(np.abs(s).max()), lim)


def check_ceiling(meas):
    total = meas["dr"] + Z_MAX * meas["dt"] + Z_MAX * 2.0 ** -24
    worst = int(np.argmax(meas["abs"]))
    assert total <= CEILING, (f"dr {meas['dr']:.3e} (octave {worst}, n = {meas['abs_at'][worst]}) + {Z_MAX} * dt {meas['dt']:.3e} "
                              f"+ {Z_MAX} * 2^-24 = {total:.3e} > {CEILING:g}")


def check_tripwires(meas):
    bad = [f"octave {e}: abs {meas['abs'][e]:.3e} > {radius_abs_limit(e):.3e}" for e in range(OCTAVES) if meas["abs"][e] > radius_abs_limit(e)]
    bad += [f"octave {e}: rel {meas['rel'][e]:.3e} > {radius_rel_limit(e):.3e}" for e in range(OCTAVES) if meas["rel"][e] > radius_rel_limit(e)]
    if meas["dt"] > trig_limit():
        bad.append(f"trig {meas['dt']:.3e} > {trig_limit():.3e}")
    if meas["dt_quarter"] > trig_quarter_limit():
        bad.append(f"trig at the quarter turns {meas['dt_quarter']:.3e} > {trig_quarter_limit():.3e}")
    assert not bad, "; ".join(bad)


def check_moments(rad, c, s, who):
    """The moments of the tables' own product distribution within what the ASSERTED pointwise limits imply."""
    ideal = reference()["m"]
    got = nr.discrete_moments(rad, c, s)
    bound = moment_bounds([radius_abs_limit(e) for e in range(OCTAVES)], trig_limit())
    bad = []
    for key in ("var", "var_s", "kurt", "kurt_s", "Ec", "Es", "Ecs"):
        dev = got[key] - ideal[key]
        print(f"[noise] {who} moment {key}: {got[key]:.11f} against {ideal[key]:.11f}: off by {dev:+.3e} (bound {bound[key]:.3e})")
        if not abs(dev) <= bound[key]:
            bad.append(f"{key} off by {dev:+.3e} > {bound[key]:.3e}")
    assert not bad, "; ".join(bad)
    return got


# ---------------------------------------------------------------------------------------------------------- the program
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

_stopped = []   # why no further run of the program is started


def run_mode(exe, out_dir, mode, *args):
    """One run of the program; the return code is looked at before anything else, and after a bad one nothing more starts."""
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    try:
        run = subprocess.run([exe, mode, str(out_dir), *map(str, args)], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _stopped.append(f"noise_domain {mode} did not end in 120 s")
        raise
    if run.returncode != 0:
        _stopped.append(f"noise_domain {mode} ended with {run.returncode}")
        pytest.fail(f"noise_domain {mode} ended with {run.returncode}:\n{run.stdout}\n{run.stderr}")
    print(run.stdout, end="")
    return run.stdout


def load(out_dir, name, dtype, count):
    v = np.fromfile(os.path.join(str(out_dir), name), dtype=dtype)
    assert v.size == count, (name, v.size, count)
    return v


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("noise_domain")
    exe = str(d / "noise_domain")
    flags = [f for f in _build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([_build.hipcc(), *flags, "-I", _build.CSRC, SRC, "-o", exe])
    return exe, d


@pytest.fixture(scope="module")
def tables(prog):
    """The device tables (one run of `radius`, one of `trig`) and their errors against float64."""
    exe, d = prog
    line = run_mode(exe, d, "radius")
    m = re.search(r"radius: (\d+) inputs, bm_u1_mul mismatches (\d+)", line)
    assert m and (int(m.group(1)), int(m.group(2))) == (nr.N_RADIUS, 0), line
    line = run_mode(exe, d, "trig")
    assert re.search(rf"trig: {nr.N_ANGLE} inputs", line), line
    rad, c, s = load(d, "radius.f32", np.float32, nr.N_RADIUS), load(d, "cos.f32", np.float32, nr.N_ANGLE), load(d, "sin.f32", np.float32, nr.N_ANGLE)
    for name in ("radius.f32", "cos.f32", "sin.f32"):
        os.remove(os.path.join(str(d), name))
    meas = measure(rad, c, s)
    report(meas, "device")
    return rad, c, s, meas


@pytest.mark.gpu
def test_known_answers_and_both_overloads(prog):
    exe, d = prog
    line = run_mode(exe, d, "kat")
    m = re.search(r"kat: words((?: [0-9a-f]{8}){24}); known-answer mismatches (\d+); overloads (\d+) inputs, mismatches (\d+)", line)
    assert m, line
    words = [int(w, 16) for w in m.group(1).split()]
    assert words == load(d, "kat.u32", np.uint32, 24).tolist()
    for v, (_, _, want) in enumerate(KAT):
        assert words[8 * v:8 * v + 4] == list(want), f"vector {v}, six arguments: {[hex(w) for w in words[8 * v:8 * v + 4]]}"
        assert words[8 * v + 4:8 * v + 8] == list(want), f"vector {v}, nine arguments: {[hex(w) for w in words[8 * v + 4:8 * v + 8]]}"
    assert (int(m.group(2)), int(m.group(3)), int(m.group(4))) == (0, 1 << 20, 0), line


@pytest.mark.gpu
def test_box_muller_is_the_product_of_the_two_tables(prog):
    exe, d = prog
    line = run_mode(exe, d, "product")
    m = re.search(r"product: (\d+) pairs, mismatches (\d+)", line)
    assert m and (int(m.group(1)), int(m.group(2))) == (4 + (1 << 24), 0), line


@pytest.mark.gpu
def test_ranges_and_ceiling_on_every_input(tables):
    rad, c, s, meas = tables
    check_ranges(rad, c, s)
    check_ceiling(meas)


@pytest.mark.gpu
def test_tripwires_per_octave_and_at_the_quarter_turns(tables):
    check_tripwires(tables[3])


@pytest.mark.gpu
def test_moments_of_the_device_distribution(tables):
    rad, c, s, _ = tables
    check_moments(rad, c, s, "device")


# -------------------------------------------------------------------------------------------- the shipped library's stream
SEED = 0x0123456789abcdef        # two different nonzero key words
FIRST = (1 << 32) - 66           # counters with c1 = 0 and with c1 = 1
N, T, K_POSTERIOR = 130, 5, 70
SOLVES = (3, 4)
R_MAX = 5                        # float4 groups of the widest row (T * 4 = 20 floats); narrower rows are its first groups


def _handle(dc):
    from mppi_playground_amd import _capi

    f4 = lambda *v: (C.c_float * 4)(*v)  # noqa: E731
    cfg = _capi.MppiConfig(model=_capi.MODEL_GENERIC, horizon=T, dim_state=2, dim_control=dc, num_samples=N, sample_offset=FIRST,
                           inherit_count=1 << 40, u_min=f4(-1, -1, -1, -1), u_max=f4(1, 1, 1, 1), sigmas=f4(1.0, 1.0, 1.0, 1.0),
                           seed=SEED, device=0)
    return _capi.Handle(cfg)


@pytest.fixture(scope="module")
def streams(prog):
    """{(solve, first): float32 [n, 4 R_MAX]} from the program's `stream` mode, with the float64 normals of the same counters."""
    exe, d = prog
    out = {}
    for solve, first, n in [(SOLVES[0], FIRST, N), (SOLVES[1], FIRST, N), (SOLVES[1], 0, K_POSTERIOR)]:
        line = run_mode(exe, d, "stream", hex(SEED), solve, first, n, R_MAX)
        assert re.search(rf"stream: {n * R_MAX * 4} floats", line), line
        dev = load(d, "stream.f32", np.float32, n * R_MAX * 4).reshape(n, 4 * R_MAX)
        ideal = nr.ideal_normals(SEED, solve, first, n, R_MAX)
        err = float(np.abs(dev - ideal).max())
        print(f"[noise] stream solve {solve} first {first}: largest so far {err:.3e} against float64 (limit {pointwise_limit():.3e})")
        assert err <= pointwise_limit(), (solve, first, err)
        out[solve, first] = dev
    assert not np.array_equal(out[SOLVES[0], FIRST], out[SOLVES[1], FIRST])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dc", [1, 2, 4])
def test_library_draws_the_stream(streams, dc):
    """mppi_sample + mppi_export_noise of a generic handle: element (i, t, k) is column t * dc + k of the row of sample
    FIRST + i, bit for bit; sigma = 1 scales exactly.  Rows of 5, 10 and 20 floats: the first two end inside a group."""
    import torch

    h = _handle(dc)
    row = T * dc
    for solve in SOLVES:
        e = torch.empty(N, T, dc, device="cuda")
        h.call("mppi_sample", solve, None)
        h.call("mppi_export_noise", e.data_ptr(), None, None)
        torch.cuda.synchronize()
        got = e.cpu().numpy().reshape(N, row)
        want = streams[solve, FIRST][:, :row]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dc, solve, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        ideal = nr.ideal_normals(SEED, solve, FIRST, N, R_MAX)[:, :row]
        assert np.abs(got - ideal).max() <= pointwise_limit()
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dc", [1, 2, 4])
def test_library_posterior_draws_the_stream(streams, dc):
    """mppi_sample_posterior with loc = 0: sample q of the k draws is counter index q (not FIRST + q) at the solve index it is
    given.  Values, not bits: loc + eps turns a -0 into +0."""
    import torch

    h = _handle(dc)
    row, solve = T * dc, SOLVES[1]
    loc = torch.zeros(row, device="cuda")
    out = torch.full((K_POSTERIOR, row), float("nan"), device="cuda")
    h.call("mppi_sample_posterior", solve, loc.data_ptr(), K_POSTERIOR, out.data_ptr(), None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, streams[solve, 0][:, :row]), dc
    ideal = nr.ideal_normals(SEED, solve, 0, K_POSTERIOR, R_MAX)[:, :row]
    assert np.abs(got - ideal).max() <= pointwise_limit()
    h.close()
