"""The growth rule of the step table behind mppi_set_discs, for both moving-disc models on a real MI355X: a longer table
reallocates the handle's buffer without losing the other writer's part, a shorter one reuses it, and a copy of the handle
carries what the source holds.  Every comparison is equality of bits."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_moving_discs as NAV
import test_gpu_racing_discs as RAC

pytestmark = pytest.mark.gpu

f32 = np.float32
T, N, IDX = 8, 64, 3


def same_bits(name, got, want):
    assert np.shape(got) == np.shape(want), f"{name}: shape {np.shape(got)} against {np.shape(want)}"
    NAV.same_bits(name, got, want)


def get_discs(h, st):
    """-> (padded table [rows, 8, 4], rows, n) of a handle"""
    rows, n = C.c_int(-1), C.c_int(-1)
    h.call("mppi_get_discs", None, C.byref(rows), C.byref(n), 1, st)
    out = torch.empty(rows.value, 8, 4, device="cuda")
    h.call("mppi_get_discs", out.data_ptr(), C.byref(rows), C.byref(n), 1, st)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rows.value, n.value


def rollout(h, st):
    h.call("mppi_sample", IDX, st)
    h.call("mppi_rollout_cost", st)
    c = torch.empty(N, device="cuda")
    h.call("mppi_get_costs", c.data_ptr(), 1, st)
    return c.cpu().numpy()


def setup(model):
    """-> (R, first table, second table, make(table) -> a fresh rig at math level 0, reference window or None)"""
    if model == "nav2d_discs":
        t1, x0 = NAV.R.case("n3", T)
        t2, _ = NAV.R.case("weights8", T)
        return NAV.R, t1, t2, (lambda table: NAV.DiscRig(table, x0, T, N, math=0)), None
    t1, x0, ref = RAC.case("n3", T)
    t2, _, _ = RAC.case("overlap2", T)
    return RAC.R, t1, t2, (lambda table: RAC.DiscRig(table, x0, ref, T, N, math=0)), ref


@pytest.mark.parametrize("model", ["nav2d_discs", "racing_discs"])
def test_longer_then_shorter_table_and_a_copy(model):
    R, t1, t2, make, ref = setup(model)
    assert t1.shape[1] != t2.shape[1]
    fresh = make(t2)
    want2 = fresh.rollout(IDX)
    fresh.close()
    rig = make(t1)
    st = rig.solver._stream()
    # 1. a T-row table from the host (racing: and a T + 1-row window)
    rig.set_table(t1)
    if ref is not None:
        assert ref.shape[0] == T + 1
        rig.set_ref(ref)
    c1 = rig.rollout(IDX)
    assert not np.array_equal(c1, want2)
    # 2. a 3T-row table from the device: the buffer is reallocated
    rest = np.tile(t2, (2, 1, 1))
    rest[:, :, 0:2] += f32(0.5)
    long = np.ascontiguousarray(np.concatenate([t2, rest]), f32)
    assert long.shape[0] == 3 * T and np.all(np.isfinite(long))
    rig.set_table(long, on_device=True)
    got, rows, n = get_discs(rig.h, st)
    assert (rows, n) == (3 * T, t2.shape[1])
    same_bits("long table: padded rows", got, R.padded(long))
    if ref is not None:
        same_bits("long table: the window survived the growth", rig.get_ref(T + 1), ref)
    c2 = rig.rollout(IDX)
    same_bits("long table: costs of a fresh handle given its first T rows", c2, want2)
    # 4. a copy of the handle after the growth
    twin = copy.deepcopy(rig.solver)
    assert twin._h is not rig.solver._h
    tw, trows, tn = get_discs(twin._h, twin._stream())
    assert (trows, tn) == (rows, n)
    same_bits("copy: padded rows", tw, got)
    same_bits("copy: costs", rollout(twin._h, twin._stream()), c2)
    twin._h.close()
    # 3. the first table again: no reallocation
    rig.set_table(t1)
    got, rows, n = get_discs(rig.h, st)
    assert (rows, n) == (T, t1.shape[1])
    same_bits("short table again: padded rows", got, R.padded(t1))
    same_bits("short table again: costs", rig.rollout(IDX), c1)
    rig.close()
