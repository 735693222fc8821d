"""The noise chain (csrc/philox.hpp: box_muller, in every kernel that draws from it) and the padded-map lookup compute
what the commit before the shorter operand forms computed, to the bit, on a real MI355X.

tests/golden/noise_and_lookup_bits.npz holds that commit's OWN outputs (recorded on the GPU by
scripts/record_noise_bits.py; not the reference's): for every case of tests/noise_bits_cases.py and two consecutive solves,
the exported noise, `costs`, `action_seq` and `state_seq`.  Every item must be byte-equal.  The cases and why these shapes:
tests/noise_bits_cases.py.
"""
import os

import numpy as np
import pytest

import noise_bits_cases as nb
from helpers import GOLDEN
from test_gpu_covariance import _need_gpu, make

pytestmark = pytest.mark.gpu
_golden = []


def golden():
    if not _golden:
        _golden.append(np.load(os.path.join(GOLDEN, "noise_and_lookup_bits.npz")))
    return _golden[0]


def same_bytes(name, got):
    z = golden()
    want_keys = sorted(k for k in z.files if k.startswith(name + "/"))
    assert want_keys == sorted(f"{name}/{k}" for k in got), name  # (nothing recorded goes unchecked)
    for key in want_keys:
        g, w = got[key.split("/", 1)[1]], z[key]
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, key
        diff = int((g.view(np.uint32) != w.view(np.uint32)).sum())
        assert diff == 0, f"{key}: {diff} of {w.size} values differ from the recorded bits ({z['label']})"


@pytest.mark.parametrize("c", nb.CASES, ids=[c["name"] for c in nb.CASES])
def test_solves(c):
    _need_gpu()
    same_bytes(c["name"], nb.run(c, make))


@pytest.mark.parametrize("g", nb.GENERIC, ids=[g["name"] for g in nb.GENERIC])
def test_generic_draw(g):
    _need_gpu()
    same_bytes(g["name"], nb.run_generic(g))


def test_the_fixture_holds_every_case():
    names = {k.split("/", 1)[0] for k in golden().files if "/" in k}
    assert names == {c["name"] for c in nb.CASES} | {g["name"] for g in nb.GENERIC}
