"""The re-rolled state trajectories of every query after a solve, on a real MI355X: `_state_seq_batch` (rollout_samples_kernel),
get_top_samples (topk_rollout_kernel: direct, select and sorted launches; noise from the block's LDS copy, regenerated in the
lane, or read from the tiles) and mppi_rollout_actions (rollout_actions_kernel), for the cases of tests/reroll_cases.py.

After one forward() per (case, math level, start, noise source):
  1. anchor   `_state_seq_batch` against the oracle's S on the exported noise (tests/mlp_ref.py in float64 on the exported
              actions for the learned models): TOL = 1e-5 of max|S|, every sample, wrapped headings compared modulo 2 pi.
              The limit is the suite's; test_reroll_cases_host.py holds the oracle's own one-ulp sensitivity under it.
              relu networks at math 0 also equal the fp32 restatement bit for bit.
  2. top      get_top_samples(k) states == `_state_seq_batch`[order[:k]] to the bit, order = the host's stable sort of
              (cost key, index) over the device's costs (ties by index: see reroll_cases.order_is_determined); weights
              within TOL of the float64 softmax of the device's costs (the temperature keeps max|c| / lambda <= 40: see
              reroll_cases.temperature); row 0 of every trajectory == the caller's x0 to the bit (but the mountain car's:
              the reference leaves its dynamics' mutated input views in the buffer, row 0 included — the anchor holds it).
  3. actions  mppi_rollout_actions on `_perturbed_action_seqs`[order[:k]] == the same rows to the bit.
  4. sources  costs and top-sample states of noise_regen = 1, noise_regen = 0 and injected noise (the first's export)
              are bit-identical.
  5. redo     starts that leave the fast paths (library-math redo of the lane), math 1 and 2: the same bit equalities,
              all three within 1e-4 (test_extreme_initial_states_against_oracle's conditioning figure) of the oracle.
Each case prints its anchor error and the model's largest so far in a `[reroll]` line (pytest -s)."""
import numpy as np
import pytest
import torch

import reroll_cases as rc
from helpers import rel_err

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
worst = {}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        d = np.abs(got.astype(f64) - want.astype(f64))
        rows = np.unique(np.nonzero(bad.reshape(bad.shape[0], -1).any(axis=1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ, in {len(rows)} of {bad.shape[0]} rows (first "
                             f"{rows[:5].tolist()}); largest difference {np.nanmax(d):.3g} = {np.nanmax(d) / max(np.abs(want).max(), 1e-30):.2e} of max|want|")


def softmax64(costs, lam):
    x = -costs.astype(f64) / lam
    e = np.exp(x - x.max())
    return e / e.sum()


def make(case, math, lam):
    """One solver per (case, math level); the noise source is switched with set_option."""
    if case.model in rc.MLP:
        from test_gpu_mlp_model import build

        solver, _ = build(rc.mlp_case(case.model), case.T, case.N, lam=lam, exploration=rc.EXPLORATION)
    else:
        from test_gpu_parity import _envs, make_solver

        solver, ctrl = make_solver(case.model, case.T, case.N, lambda_=lam, exploration=rc.EXPLORATION)
        if ctrl is not None:  # racing: the reference window as in test_edge_sizes_against_oracle
            env = _envs["racing"]
            ref, _ = ctrl.calc_ref_trajectory(env._robot_state, env.racing_center_path, 0, case.T, DL=0.1,
                                              lookahead_distance=3, reference_path_interval=0.85)
            assert np.array_equal(ref.numpy(), rc.racing_reference(case.T))  # (what the host chose the temperature on)
            ctrl.set_reference(ref)
    solver.set_option("math", math)
    return solver


def solve(solver, source, x0, mean, eps=None):
    solver.set_warm_start(mean)
    solver._solve_idx = rc.SOLVE_IDX
    if source == "inject":
        solver.inject_noise(torch.from_numpy(eps))
    else:
        solver.set_option("noise_regen", 1 if source == "regen" else 0)
    solver.forward(torch.from_numpy(x0))


def top_states(solver, k):
    ts, tw = solver.get_top_samples(k)
    return ts.cpu().numpy(), tw.cpu().numpy()  # (pooled buffers: copied before the next query)


def rollout_actions(solver, U, x0):
    a = torch.from_numpy(np.ascontiguousarray(U, f32)).cuda()
    x = torch.from_numpy(x0).cuda()
    out = torch.empty(len(U), solver._horizon + 1, solver._dim_state, device="cuda")
    solver._h.call("mppi_rollout_actions", a.data_ptr(), len(U), x.data_ptr(), out.data_ptr(), solver._stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_case(case, math, xs, sources, anchor_tol):
    model, T, N = case.model, case.T, case.N
    hs = [rc.host_solve(case.name, model, T, N, s) for s in xs]
    lam = max(h["lam"] for h in hs)
    solver = make(case, math, lam)
    for h in hs:
        x0, mean = h["x0"], h["mean"]
        tag = f"{case.name} math {math} x0 {x0.tolist()}"
        solve(solver, sources[0], x0, mean)
        eps = solver._action_noises.cpu().numpy()
        c = solver._costs.cpu().numpy()
        tops = {k: top_states(solver, k) for k in case.ks}
        batch = solver._state_seq_batch.cpu().numpy()
        U = solver._perturbed_action_seqs.cpu().numpy()
        assert np.all(np.isfinite(c)) and np.all(np.isfinite(batch)), tag
        assert np.array_equal(bits(U), bits(rc.clamped_actions(model, mean, eps, N))), tag

        # 1. anchor
        if model in rc.MLP:
            _, S = rc.reference_states(model, T, N, x0, mean, eps, U=U, dtype=f64)
            if math == 0:
                same_bits(f"{tag}: _state_seq_batch against the fp32 restatement", batch,
                          rc.reference_states(model, T, N, x0, mean, eps, U=U)[1])
        else:
            _, S = rc.reference_states(model, T, N, x0, mean, eps)
        err = rc.state_error(model, batch, S)
        worst[model] = max(worst.get(model, 0.0), err)
        print(f"[reroll] {tag}: anchor {err:.2e} of max|S| (limit {anchor_tol:.0e}); {model} so far {worst[model]:.2e}")
        assert err < anchor_tol, (tag, err)

        # 2. top samples are rows of that batch; 3. so are the re-rolled explicit actions
        row0 = model not in rc.ROW0_MUTATED
        if row0:
            same_bits(f"{tag}: row 0 of _state_seq_batch against x0", batch[:, 0, :], np.broadcast_to(x0, (N, len(x0))))
        assert np.abs(c).max() / lam <= 40.0, (tag, np.abs(c).max(), lam)  # (reroll_cases.temperature: the weights' conditioning)
        order, keys = rc.host_order(c)
        w64 = softmax64(c, lam)
        for k in case.ks:
            assert rc.order_is_determined(keys, order, k, rc.geometry(model, T, N, k)["launch"]), (tag, k)
            ts, tw = tops[k]
            same_bits(f"{tag}: get_top_samples({k}) against _state_seq_batch[order]", ts, batch[order[:k]])
            if row0:
                same_bits(f"{tag}: get_top_samples({k}) row 0 against x0", ts[:, 0, :], np.broadcast_to(x0, (k, len(x0))))
            assert tw.shape == (k,) and rel_err(tw, w64[order[:k]]) < rc.TOL, (tag, k, rel_err(tw, w64[order[:k]]))
            same_bits(f"{tag}: mppi_rollout_actions of the top {k} against _state_seq_batch[order]",
                      rollout_actions(solver, U[order[:k]], x0), batch[order[:k]])
            if anchor_tol != rc.TOL:  # the redo cases: each of the three against the oracle as well
                assert rc.state_error(model, ts, S[order[:k]]) < anchor_tol, (tag, k)

        # 4. the other noise sources see the same eps: same costs, same top samples
        for source in sources[1:]:
            solve(solver, source, x0, mean, eps)
            same_bits(f"{tag}: costs of {source} against {sources[0]}", solver._costs.cpu().numpy(), c)
            assert np.array_equal(bits(solver._action_noises.cpu().numpy()), bits(eps)), (tag, source)
            for k in case.ks:
                ts, tw = top_states(solver, k)
                same_bits(f"{tag}: get_top_samples({k}) of {source} against {sources[0]}", ts, tops[k][0])
                assert rel_err(tw, w64[order[:k]]) < rc.TOL, (tag, source, k)


@pytest.mark.parametrize("math", rc.MATHS)
@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_rerolled_trajectories(case, math):
    check_case(case, math, range(len(rc.starts(case.model))), rc.NOISE_SOURCES, rc.TOL)


@pytest.mark.parametrize("math", rc.REDO_MATHS)
@pytest.mark.parametrize("case", rc.REDO_CASES, ids=lambda c: c.name)
def test_fast_path_redo(case, math):
    """Starts whose lanes leave the fast paths: every query must hand back the library-math walk, not the fast one."""
    check_case(case, math, [case.x0], ("regen",), rc.REDO_TOL)
