"""The operands of box_muller (csrc/philox.hpp) are formed in fewer instructions than before; both new forms are the old
numbers to the bit.

* u1 = ((a >> 8) + 1) * 2^-24 is fma((float)(a >> 8), 2^-24, 2^-24) (bm_u1_fma).  n = a >> 8 < 2^24 converts exactly, the
  scale is a power of two and (n + 1) * 2^-24 is representable — n + 1 needs more than 24 bits only when it IS 2^24 — so the
  FMA's single rounding rounds nothing.  Callers without a register for the constant keep the old form (bm_u1_mul).
* the angle 0x3f800000 | (b >> 9) is the funnel shift alignbit(0x7f, b, 9) (bm_angle): the low word of (0x7f:b) >> 9.

On the GPU a small program (tests/gpu_progs/box_muller_identity.hip, built here with the library's own flags) compares the old
forms, restated literally, with the forms philox.hpp ships for EVERY input: all 2^24 values of a >> 8 and all 2^23 values
of b >> 9, each with the discarded low bits all zero and all one.  Expected mismatches: 0.  The host twins show the u1
identity in float64, where both sides are exact, over the same 2^24 values, and restate the funnel shift with 64-bit integers.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from mppi_playground_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gpu_progs", "box_muller_identity.hip")


def test_u1_identity_is_exact_in_float64():
    """(n + 1) * 2^-24 and fma(n, 2^-24, 2^-24) for all n < 2^24: every intermediate is exact in float64 (n * 2^-24 is a
    scaling, the sum has at most 25 significant bits), so float64 evaluates both sides without rounding; the value must
    also survive the round trip through float32, which is the statement that the float32 FMA rounds nothing."""
    n = np.arange(1 << 24, dtype=np.uint32)
    as_f32 = n.astype(np.float32)
    assert np.array_equal(as_f32.astype(np.uint32), n)  # the conversion is exact
    old = (n.astype(np.float64) + 1.0) * 2.0 ** -24  # exact: the sum is an integer <= 2^24, the product a scaling
    new = as_f32.astype(np.float64) * 2.0 ** -24 + 2.0 ** -24  # the FMA's infinitely precise value
    assert np.array_equal(old, new)
    assert np.array_equal(new.astype(np.float32).astype(np.float64), new)  # representable: the one rounding rounds nothing
    # the old form's two float32 operations: (float)(n + 1) is exact (n + 1 <= 2^24), the product a scaling
    old32 = (n.astype(np.uint64) + 1).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(old32.view(np.uint32), new.astype(np.float32).view(np.uint32))
    assert old32[0] == np.float32(2.0 ** -24) and old32[-1] == np.float32(1.0)  # u1 in (0, 1]


def test_angle_identity_on_the_host():
    """alignbit(0x7f, b, 9) = low word of ((0x7f << 32) | b) >> 9 on the edges, every b >> 9 with zero low bits (2^23
    values) and a random million of b."""
    rng = np.random.default_rng(19)
    b = np.concatenate([np.array([0, 1, 0x1ff, 0x200, 0x7fffffff, 0x80000000, 0xfffffe00, 0xffffffff], np.uint64),
                        np.arange(1 << 23, dtype=np.uint64) << np.uint64(9),
                        rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64)])
    new = (((np.uint64(0x7f) << np.uint64(32)) | b) >> np.uint64(9)) & np.uint64(0xffffffff)
    old = np.uint64(0x3f800000) | (b >> np.uint64(9))
    assert np.array_equal(old, new)
    as_float = new.astype(np.uint32).view(np.float32)
    assert as_float.min() == 1.0 and as_float.max() < 2.0  # 1 + u2 in [1, 2)


@pytest.mark.gpu
def test_every_input_on_the_device(tmp_path):
    exe = str(tmp_path / "box_muller_identity")
    flags = [f for f in _build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([_build.hipcc(), *flags, "-I", _build.CSRC, SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    m = re.search(r"u1 (\d+) inputs, mismatches (\d+) \(four-instruction form: (\d+)\); angle (\d+) inputs, mismatches (\d+)",
                  run.stdout)
    assert m, (run.returncode, run.stdout, run.stderr)
    n_u1, bad_u1, bad_mul, n_angle, bad_angle = map(int, m.groups())
    assert (n_u1, n_angle) == (2 << 24, 2 << 23)
    assert (bad_u1, bad_mul, bad_angle) == (0, 0, 0)
    assert run.returncode == 0
