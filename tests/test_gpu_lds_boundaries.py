"""The kernels that carve up dynamic LDS (csrc/mppi_lds.hpp) at the smallest shapes where a region boundary is tight, on a
real MI355X.  Every case is an equality the suite already asserts at larger shapes: here the rows are one to three steps long,
so a region that starts a float early or a launch that asks for a float too few changes bits.

  rollout, rider block   pendulum T = 1 (R = 1, no step rows: the 8 floats of the sample blocks are fewer than the rider's
                         row + 8 = 9, the rider decides the launch's size) and T = 2: the lazily completed state sequence
                         against the eager twin's, three solves
  rollout, step rows     racing T = 3 (row 6, R = 2, 8 floats per step row): regenerated noise against tiles, and the same
                         with the control-cost term (one more region in front of the step rows)
  single launch          fused_solve 2 against 0 at N = 64 and T = 1, 3, and T = 3 with the widest filter the horizon admits
  finalize               T = 2 with the widest filter, partial rows folded in the kernel against summarize_kernel
  get_top_samples        T = 1, k = 1 and 64: the block's regenerated noise behind the two mean rows against tiles
"""
import numpy as np
import pytest
import torch

import fused_cases as fc
from test_gpu_action_cost import Rig, measure
from test_gpu_covariance import TOL, make, weights64
from test_gpu_fused_geometry import _cu, assert_single_launch, took
from test_gpu_rollout_drain import check

pytestmark = pytest.mark.gpu


def widest_window(T):
    """The widest Savitzky-Golay window mppi_set_sg_filter admits at horizon T: odd, <= 255, window / 2 <= 2T - 1."""
    return min(255, 2 * (2 * T - 1) + 1)


def filter_bound(coeffs, hist, scale, lim):
    """How far two filtered sequences [T] (one control) may lie apart when the unfiltered ones differ by at most lim * scale
    per element and the histories are equal.  The filter is linear: a' = F [history (T - 1); a (T)], F from the host
    statement of the filter applied to unit vectors, so the difference of the inputs arrives as at most |F| (lim * scale).
    Each side also rounds its own window-long fp32 accumulation: at most (window + 1) * 2^-24 * sum |c_j y_j| per side, with
    |a| <= scale (a is the weighted mean of U, scale that of |U|)."""
    from pi_mpc import _host

    T, n = len(scale), 2 * len(scale) - 1
    F = np.zeros((T, n))
    for i in range(n):
        e = np.zeros((n, 1), np.float32)
        e[i] = 1.0
        F[:, i] = _host.sg_filter_sequence(e[:T - 1], e[T - 1:], coeffs)[:, 0]
    moved = np.concatenate([np.zeros(T - 1), lim * scale])
    size = np.concatenate([np.abs(hist), scale])
    return np.abs(F) @ (moved + 2.0 * (len(coeffs) + 1) * 2.0 ** -24 * size)


@pytest.mark.parametrize("T", [1, 2])
def test_rider_block_where_it_decides_the_launch_size(T):
    N = 256
    lazy, x0 = make("pendulum", T, N, 1.0, lazy_state_seq=True)
    eager, _ = make("pendulum", T, N, 1.0)
    assert lazy._lazy_state and not eager._lazy_state
    for s in (lazy, eager):
        s.set_option("fused_solve", 0)  # (the rider block belongs to the multi-kernel path's rollout launch)
    x, kept = x0.cuda(), []
    for k in range(3):
        a, s = lazy.forward(x)
        b, sb = eager.forward(x)
        assert torch.equal(a, b), k
        kept.append((s, sb))  # (not read yet: solves 0 and 1 ride in the next solve's rollout launch)
        x = sb[0, 1].clone()
    for k, (s, sb) in enumerate(kept):  # (... and solve 2 is completed by its own one-wave kernel)
        assert torch.isfinite(sb).all(), k
        assert torch.equal(s, sb), k


def test_racing_three_steps_regenerated_noise_equals_tiles():
    check(lambda: make("racing", 3, 256, 1.0))


def test_racing_three_steps_with_the_control_cost_term():
    rig = Rig("racing", 3, 256)
    _, c1, _, _ = measure("racing_T3_regen", rig)
    rig.h.call("mppi_set_option", b"noise_regen", 0)
    _, c1t, _, _ = measure("racing_T3_tiles", rig)
    assert np.array_equal(c1.view(np.uint32), c1t.view(np.uint32))
    rig.close()


@pytest.mark.parametrize("T,sg", [(1, False), (3, False), (3, True)], ids=["T1", "T3", "T3-sg"])
def test_single_launch_against_the_multi_kernel_path(T, sg):
    N, lam = 64, 20.0
    kw = dict(use_sg_filter=True, sg_window_size=widest_window(T), sg_poly_order=3) if sg else {}
    fused, x0 = make("pendulum", T, N, lam, **kw)
    multi, _ = make("pendulum", T, N, lam, **kw)
    fused.set_option("fused_solve", 2)
    multi.set_option("fused_solve", 0)
    if sg:
        assert fused._sg_on_device and multi._sg_on_device and fused._sg_window_size == 11
    G, spb = fc.geometry(N, _cu(), mode=2, row=T)
    lim = fc.limit(G, spb, fc.row_shape(T, 1)[0], TOL)
    x = x0.cuda()
    for k in range(3):
        name = f"T{T}{' sg' if sg else ''} tick {k}"
        if k:
            multi.set_warm_start(fused._previous_action_seq.cpu().numpy(), fused._actions_history_for_sg if sg else None)
        hist = np.asarray(fused._actions_history_for_sg, np.float64).ravel() if sg else None  # (what this solve's filter reads)
        a1, s1 = fused.forward(x)
        a2, s2 = multi.forward(x)
        assert_single_launch(fused._h, N, name, mode=2, row=T)
        assert took(multi._h) == (0, 0), name
        costs = fused._costs.cpu().numpy()
        assert np.array_equal(costs, multi._costs.cpu().numpy()), name
        assert fused.last_stats()["cmin"] == multi.last_stats()["cmin"] == costs.min(), name
        # test_alternating_paths_hand_the_minimum_slot_over's limit on the weighted sums, relative to the column's scale
        U = fused._perturbed_action_seqs.cpu().numpy().reshape(N, -1).astype(np.float64)
        w = weights64(costs, lam)[0]
        scale = (w @ np.abs(U)) / w.sum()
        bound = lim * scale
        if sg:  # ... carried through the filter, which both paths run on equal histories (see filter_bound)
            bound = filter_bound(fused._coeffs, hist, scale, lim)
        err = float(np.max(np.abs(a1.cpu().numpy().ravel().astype(np.float64) - a2.cpu().numpy().ravel()) / bound))
        print(f"[lds] fused {name}: action vs the multi-kernel twin at {err:.3e} of its bound (weighted sums: {lim:.3e} of the scale)")
        assert err <= 1.0, f"{name}: {err:.3e} of the bound"
        x = s1[0, 1].clone()


def test_finalize_folds_with_the_widest_filter():
    """fold_path 1 (finalize_kernel folds the partial rows: group sums behind the filter staging) against 2 (summarize_kernel):
    one summation tree, so statistics, action, state sequence and filter history are bit-identical."""
    T, N = 2, 256
    kw = dict(use_sg_filter=True, sg_window_size=widest_window(T), sg_poly_order=3)
    outs = []
    for path in (1, 2):
        solver, x0 = make("pendulum", T, N, 1.0, **kw)
        assert solver._sg_on_device and solver._sg_window_size == 7
        solver.set_option("fused_solve", 0)
        solver.set_option("fold_path", path)
        x, out = x0.cuda(), []
        for _ in range(3):
            a, s = solver.forward(x)
            st = solver.last_stats()
            out += [a.clone(), torch.as_tensor(s).clone(), torch.tensor([st[k] for k in sorted(st)], dtype=torch.float64),
                    torch.as_tensor(np.asarray(solver._actions_history_for_sg, np.float32))]
            x = torch.as_tensor(s)[0, 1].clone()
        outs.append(out)
    for i, (x, y) in enumerate(zip(*outs)):
        assert torch.isfinite(x).all(), i
        assert torch.equal(x.cpu(), y.cpu()), i


@pytest.mark.parametrize("k", [1, 64])
def test_top_samples_of_a_one_step_row(k):
    outs = []
    for regen in (1, 0):
        solver, x0 = make("pendulum", 1, 256, 1.0)
        solver.set_option("noise_regen", regen)
        solver.set_option("fused_solve", 0)
        solver.forward(x0.cuda())
        states, weights = solver.get_top_samples(k)
        outs.append((solver._costs.clone(), torch.as_tensor(states).clone(), torch.as_tensor(weights).clone()))
    for x, y in zip(*outs):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y)
    assert outs[0][1].shape[0] == k
