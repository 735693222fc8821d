"""The floor-based heading wrap of the FAST racing / nav2d / goal-zone step (mppi_models.inc: wrap_inc_f) against the
branchy sequence it replaced, bit for bit, on a dense boundary-heavy subset of its domain: every float within 2^16 ulps
of the points where the branch changes (fl(x + pi) = 0 and 2pi) and of 0, +-pi, +-2pi, plus random headings +
increments.  The exhaustive proof over every float of [-2pi, 2pi] is scripts/enum/enum_wrap_index.cpp (recorded output:
profiles/r07_enum_wrap_index.txt)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

F32 = np.float32
PI = F32(3.14159274)
TWO_PI = F32(6.28318548)
_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul", "wrap_probe.cpp")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("wrap_probe") / "libwrap_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, _SRC])
    lib = C.CDLL(so)
    lib.probe_wrap_inc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]

    def run(x):
        x = np.ascontiguousarray(x, dtype=F32)
        s, f = np.empty_like(x), np.empty_like(x)
        lib.probe_wrap_inc(x.ctypes.data, s.ctypes.data, f.ctypes.data, x.size)
        return s, f
    return run


def branchy_wrap(x):
    """The sequence of rounds 1-6, in float32: a = x + pi; a >= 2pi -> a - 2pi; r < 0 -> r + 2pi; r - pi."""
    with np.errstate(all="ignore"):
        a = (x + PI).astype(F32)
        r = np.where(a >= TWO_PI, (a - TWO_PI).astype(F32), a)
        r = np.where(r < 0, (r + TWO_PI).astype(F32), r)
        return (r - PI).astype(F32)


def neighbours(anchors, k):
    """Every float within k ulps of each anchor (walking the bit patterns through zero on both sides)."""
    out = []
    for a in np.asarray(anchors, F32):
        b = int(a.view(np.int32))
        key = b if b >= 0 else -(b & 0x7FFFFFFF)
        keys = np.arange(key - k, key + k + 1, dtype=np.int64)
        u = np.where(keys >= 0, keys, (-keys) | 0x80000000).astype(np.uint32)
        out.append(u.view(F32))
    return np.concatenate(out)


def test_wrap_inc_boundaries_bit_identical(probe):
    # x where fl(x + pi) crosses 0 (x ~ -pi) and 2pi (x ~ pi), the domain's ends (+-2pi) and 0
    x = neighbours([-PI, PI, F32(TWO_PI - PI), -TWO_PI, TWO_PI, 0.0, F32(-0.0)], 1 << 16)
    x = x[np.abs(x) <= TWO_PI]
    s, f = probe(x)
    ref = branchy_wrap(x)
    assert np.array_equal(s.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(f.view(np.uint32), ref.view(np.uint32))


def test_wrap_inc_heading_plus_increment_bit_identical(probe):
    rng = np.random.default_rng(7)
    th = ((rng.random(2_000_000) * 2 - 1) * np.pi).astype(F32)
    th = th[(th >= -PI) & (th < PI)]
    inc = ((rng.random(th.size) * 2 - 1) * np.pi).astype(F32)
    x = (th + inc).astype(F32)
    s, f = probe(x)
    ref = branchy_wrap(x)
    assert np.array_equal(s.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(f.view(np.uint32), ref.view(np.uint32))
    # the result is a wrapped heading: [-pi, pi]
    assert np.all((f >= -PI) & (f <= PI))
