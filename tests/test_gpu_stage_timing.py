"""Stage timing (option "timing") on a real MI355X: the event pair of a timed stage rides on the stage's own dispatches
(csrc/mppi_handle.hpp, StageTimer) instead of bracketing it with marker packets on the stream.

What is held here: timing never changes a result (bit identity across timing = 0 / 1 / 2, a full event pool, a captured
solve); a stage reports one pair per solve and a time between 0 and the wall time of a solve; the dispatch-bound rollout time
is below what plain stream markers around the same launch see; a two-launch stage spans both of its launches.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from test_gpu_covariance import make

pytestmark = pytest.mark.gpu

STAGES = ("sample", "rollout_cost", "weights_reduce", "finalize")
POOL_PAIRS = 8192  # StageTimer keeps at most 16 384 events per stage


def drain(solver):
    """({stage: mean ms}, {stage: pairs}) since the last drain (mppi_get_timing: four means, then four counts)."""
    out = (C.c_float * 8)()
    solver._h.call("mppi_get_timing", out)
    return {n: float(out[i]) for i, n in enumerate(STAGES)}, {n: int(out[4 + i]) for i, n in enumerate(STAGES)}


def closed_loop(solver, x0, steps=3):
    """`steps` solves, each from the state the last plan reaches first: every (action_seq, state_seq), copied."""
    x, outs = x0.cuda(), []
    for _ in range(steps):
        a, s = solver.forward(x)
        outs.append((a.clone(), torch.as_tensor(s).clone()))
        x = outs[-1][1][0, 1].clone()
    torch.cuda.synchronize()
    return outs


def same_bits(got, want):
    return len(got) == len(want) and all(torch.equal(a, b) and torch.equal(s, t) for (a, s), (b, t) in zip(got, want))


def test_racing_solves_are_bit_identical_under_every_timing_mode():
    """N = 8192 is above the single launch's limit: rollout, reduction and finalize run as three kernels."""
    outs = []
    for timing in (0, 1, 2):
        solver, x0 = make("racing", 8, 8192, 1.0)
        solver.set_option("timing", timing)
        outs.append(closed_loop(solver, x0))
        _, counts = drain(solver)
        want = {0: (0, 0, 0, 0), 1: (0, 3, 3, 3), 2: (0, 3, 0, 0)}[timing]  # (the noise is regenerated: `sample` launches nothing)
        assert tuple(counts[n] for n in STAGES) == want, (timing, counts)
    assert same_bits(outs[1], outs[0]) and same_bits(outs[2], outs[0])


def test_pendulum_solves_are_bit_identical_under_every_timing_mode():
    """N = 256 is one launch under timing = 0 and 2 (the pair rides on solve_fused_kernel); timing = 1 declines the single
    launch, so that solver is held to a twin that never takes it."""
    outs = {}
    for name, timing, fused in (("t0", 0, 1), ("t2", 2, 1), ("t1", 1, 1), ("three_kernels", 0, 0)):
        solver, x0 = make("pendulum", 15, 256, 1.0)
        solver.set_option("timing", timing)
        solver.set_option("fused_solve", fused)
        outs[name] = closed_loop(solver, x0)
        _, counts = drain(solver)
        want = {"t0": (0, 0, 0, 0), "t2": (0, 3, 0, 0), "t1": (0, 3, 3, 3), "three_kernels": (0, 0, 0, 0)}[name]
        assert tuple(counts[n] for n in STAGES) == want, (name, counts)
    assert same_bits(outs["t2"], outs["t0"])
    assert same_bits(outs["t1"], outs["three_kernels"])


@pytest.mark.parametrize("model,T,N,regen,lazy", [("racing", 8, 8192, 1, False), ("pendulum", 15, 256, 0, False),
                                                  ("racing", 8, 8192, 1, True)])
def test_stage_times_are_sane(model, T, N, regen, lazy):
    """20 solves with timing = 1: one pair per solve for every stage that ran, each mean above 0 and below the wall time of a
    solve.  Then 20 rollout launches of the same solver, each also bracketed by plain stream markers (torch.cuda.Event): the
    markers include the wait between marker and dispatch, the dispatch-bound pair does not, so the latter is the smaller."""
    solver, x0 = make(model, T, N, 1.0, **({"lazy_state_seq": True} if lazy else {}))
    solver.set_option("noise_regen", regen)  # (0: the noise tiles are materialised, so `sample` launches sample_kernel)
    solver.set_option("timing", 1)
    x0 = x0.cuda()
    solver.forward(x0)
    torch.cuda.synchronize()
    drain(solver)
    solver.stage_times_ms()  # (also drains the stand-alone state-sequence stage of the lazy case)
    t0 = time.perf_counter()
    for _ in range(20):
        a, s = solver.forward(x0)
        if lazy:
            s.clone()  # read at once: the stand-alone state_seq_kernel completes it
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) / 20 * 1e3
    if lazy:
        st = solver.stage_times_ms()
        print(f"{model} lazy: state_seq_standalone {st['state_seq_standalone'] * 1e3:.2f} us x {st['state_seq_standalone_launches']:.0f}, "
              f"wall {wall_ms * 1e3:.1f} us per solve")
        assert st["state_seq_standalone_launches"] == 20.0 and 0.0 < st["state_seq_standalone"] < wall_ms, st
        return
    ms, counts = drain(solver)
    print(f"{model} N={N}: " + ", ".join(f"{n} {ms[n] * 1e3:.2f} us x {counts[n]}" for n in STAGES) + f", wall {wall_ms * 1e3:.1f} us per solve")
    ran = STAGES if not regen else STAGES[1:]
    for n in STAGES:
        if n in ran:
            assert counts[n] == 20 and 0.0 < ms[n] < wall_ms, (n, ms, counts, wall_ms)
        else:
            assert counts[n] == 0 and ms[n] == -1.0, (n, ms, counts)
    st = solver._stream()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for e0, e1 in pairs:
        e0.record()
        solver._h.call("mppi_rollout_cost", st)
        e1.record()
    torch.cuda.synchronize()
    markers_ms = float(np.mean([e0.elapsed_time(e1) for e0, e1 in pairs]))
    ms, counts = drain(solver)
    print(f"{model} N={N}: rollout dispatch-bound {ms['rollout_cost'] * 1e3:.2f} us, between stream markers {markers_ms * 1e3:.2f} us")
    assert counts["rollout_cost"] == 20 and 0.0 < ms["rollout_cost"] < markers_ms, (ms, markers_ms)


def test_a_two_launch_stage_spans_both_launches():
    """fold_path = 2 forces summarize_kernel behind weights_reduce_kernel: still one pair per solve (start on the first
    dispatch, stop on the second), and a time no smaller than the reduction alone (fold_path = 1) less that figure's own spread."""
    times = {}
    for fold in (1, 2):
        solver, x0 = make("racing", 8, 8192, 1.0)
        solver.set_option("fold_path", fold)
        solver.set_option("timing", 1)
        x0 = x0.cuda()
        solver.forward(x0)
        torch.cuda.synchronize()
        drain(solver)
        per_solve = []
        for _ in range(20):
            solver.forward(x0)
            torch.cuda.synchronize()
            ms, counts = drain(solver)
            assert counts["weights_reduce"] == 1, counts
            per_solve.append(ms["weights_reduce"])
        times[fold] = np.asarray(per_solve)
        assert (times[fold] > 0.0).all()
    spread = float(times[1].max() - times[1].min())
    print(f"weights_reduce: fold_path=1 {times[1].mean() * 1e3:.2f} us (spread {spread * 1e3:.2f}), fold_path=2 {times[2].mean() * 1e3:.2f} us")
    assert times[2].mean() >= times[1].mean() - spread


def test_a_full_event_pool_leaves_later_solves_untimed_and_unchanged():
    """More timed solves than the pool holds pairs, never drained: no error, the same bits as an untimed twin, and exactly the
    pool's pairs reported.  (The smallest single-launch problem: 8200 solves take about a second.)"""
    timed, x0 = make("pendulum", 5, 64, 1.0)
    twin, _ = make("pendulum", 5, 64, 1.0)
    timed.set_option("timing", 2)
    x0 = x0.cuda()
    for k in range(POOL_PAIRS + 8):
        a, s = timed.forward(x0)
        b, t = twin.forward(x0)
        if k % 1024 == 0 or k >= POOL_PAIRS - 2:  # (now and then, and across the solve that finds the pool full)
            assert torch.equal(a, b) and torch.equal(torch.as_tensor(s), torch.as_tensor(t)), k
    torch.cuda.synchronize()
    ms, counts = drain(timed)
    assert tuple(counts[n] for n in STAGES) == (0, POOL_PAIRS, 0, 0), counts
    assert ms["rollout_cost"] > 0.0, ms
    a, s = timed.forward(x0)  # (drained: timed again)
    b, t = twin.forward(x0)
    assert torch.equal(a, b) and torch.equal(torch.as_tensor(s), torch.as_tensor(t))
    assert drain(timed)[1]["rollout_cost"] == 1


def test_a_captured_solve_with_timing_replays_to_the_eager_result():
    """A stream that is being captured keeps plain event records around the stage: the captured solve replays to what an
    eager twin returns."""
    solver, x0 = make("racing", 8, 8192, 1.0)
    twin, _ = make("racing", 8, 8192, 1.0)
    solver.set_option("timing", 2)
    x0 = x0.cuda()
    for _ in range(3):
        solver.forward(x0)
        twin.forward(x0)
    a_t, s_t = twin.forward(x0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            a, s = solver.forward(x0)
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, a_t) and torch.equal(torch.as_tensor(s), torch.as_tensor(s_t))
    del g
