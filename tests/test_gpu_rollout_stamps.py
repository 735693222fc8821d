"""The rollout stage timed from inside its kernel on a real MI355X: rollout_cost_kernel writes a pair of wall-clock stamps
(block 0 the start, every block an atomicMax into the end) instead of carrying a pair of events on its dispatch
(csrc/mppi_handle.hpp, StageTimer; option "timing_source" = 1 brings the events back).

What is held here: a stamped solve returns the bits of an untimed one (also past a full stamp pool, and with the rider
block of a lazy state sequence in the launch); the stage reports one pair per launch and a time above 0, below the wall
time of a solve and no larger than what the events on the dispatch see; the time grows with the horizon; a drain re-arms
the pairs it read.

Shapes: racing, T = 8, N = 8192 (128 tiles, 32 blocks, above the single launch's limit) and the ragged N = 8192 + 37 (a last
tile partly past the end, a last block with fewer than four live waves).
"""
import ctypes as C
import time

import pytest
import torch

from test_gpu_covariance import make

pytestmark = pytest.mark.gpu

STAGES = ("sample", "rollout_cost", "weights_reduce", "finalize")
POOL_PAIRS = 8192  # the stamp pool is as deep as the event pool


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


def rollout_launches(solver, n=20):
    """`n` launches of the rollout stage alone, then a drain: (mean ms, pairs) of the stage."""
    st = solver._stream()
    for _ in range(n):
        solver._h.call("mppi_rollout_cost", st)
    torch.cuda.synchronize()
    ms, counts = drain(solver)
    return ms["rollout_cost"], counts["rollout_cost"]


@pytest.mark.parametrize("N", [8192, 8192 + 37])
def test_stamped_solves_are_bit_identical_to_untimed_ones(N):
    """timing = 2 against a timing = 0 twin over three closed-loop solves; then 20 solves: one pair each, nothing for the other
    stages, and a mean above 0 and below the wall time of a solve."""
    outs = {}
    for timing in (0, 2):
        solver, x0 = make("racing", 8, N, 1.0)
        solver.set_option("timing", timing)
        outs[timing] = closed_loop(solver, x0)
        _, counts = drain(solver)
        assert tuple(counts[n] for n in STAGES) == ((0, 3, 0, 0) if timing else (0, 0, 0, 0)), (timing, counts)
    assert same_bits(outs[2], outs[0])
    x0 = x0.cuda()
    t0 = time.perf_counter()
    for _ in range(20):
        solver.forward(x0)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) / 20 * 1e3
    ms, counts = drain(solver)
    print(f"racing N={N} T=8: stamped rollout {ms['rollout_cost'] * 1e3:.2f} us x {counts['rollout_cost']}, wall {wall_ms * 1e3:.1f} us per solve")
    assert tuple(counts[n] for n in STAGES) == (0, 20, 0, 0), counts
    assert 0.0 < ms["rollout_cost"] < wall_ms, (ms, wall_ms)


def test_the_stamped_time_is_no_larger_than_the_event_time():
    """One solver, 20 rollout launches stamped, then 20 with the events on the dispatch: the stamps lie inside the dispatch."""
    solver, x0 = make("racing", 8, 8192, 1.0)
    solver.set_option("timing", 2)
    solver.forward(x0.cuda())
    torch.cuda.synchronize()
    drain(solver)
    stamped_ms, n0 = rollout_launches(solver)
    solver.set_option("timing_source", 1)
    rollout_launches(solver)  # (the events are created on first use: not inside the figure)
    event_ms, n1 = rollout_launches(solver)
    print(f"racing N=8192 T=8: rollout stamped {stamped_ms * 1e3:.2f} us, events on the dispatch {event_ms * 1e3:.2f} us")
    assert n0 == 20 and n1 == 20
    assert 0.0 < stamped_ms <= event_ms, (stamped_ms, event_ms)


def test_the_stamped_time_grows_with_the_horizon():
    """T = 32 is four times the steps of T = 8 in the same kernel at the same N: a pair that is never re-armed, or read from
    the wrong slot, does not show that."""
    means = {}
    for T in (8, 32):
        solver, x0 = make("racing", T, 8192, 1.0)
        solver.set_option("timing", 2)
        solver.forward(x0.cuda())
        torch.cuda.synchronize()
        drain(solver)
        means[T], n = rollout_launches(solver)
        assert n == 20
    print(f"racing N=8192: stamped rollout T=8 {means[8] * 1e3:.2f} us, T=32 {means[32] * 1e3:.2f} us")
    assert 0.0 < means[8] < means[32], means


def test_a_drain_re_arms_the_pairs_it_read():
    solver, x0 = make("racing", 8, 8192, 1.0)
    solver.set_option("timing", 2)
    x0 = x0.cuda()
    for _ in range(5):
        solver.forward(x0)
    torch.cuda.synchronize()
    assert drain(solver)[1]["rollout_cost"] == 5
    t0 = time.perf_counter()
    solver.forward(x0)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    ms, counts = drain(solver)
    assert counts["rollout_cost"] == 1 and 0.0 < ms["rollout_cost"] < wall_ms, (ms, counts, wall_ms)
    ms, counts = drain(solver)
    assert counts["rollout_cost"] == 0 and ms["rollout_cost"] == -1.0, (ms, counts)


def test_a_full_stamp_pool_leaves_later_solves_untimed_and_unchanged():
    """More stamped solves than the pool holds pairs, never drained: no error, the bits of an untimed twin, exactly the pool's
    pairs reported, and timed again after the drain."""
    timed, x0 = make("racing", 2, 8192, 1.0)
    twin, _ = make("racing", 2, 8192, 1.0)
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
    a, s = timed.forward(x0)
    b, t = twin.forward(x0)
    assert torch.equal(a, b) and torch.equal(torch.as_tensor(s), torch.as_tensor(t))
    assert drain(timed)[1]["rollout_cost"] == 1


@pytest.mark.parametrize("timing", [2, 1])
def test_the_rider_block_of_a_lazy_state_sequence_stamps_too(timing):
    """lazy_state_seq: the state sequence of a solve rides in one extra block of the next rollout launch, which is stamped like
    any other.  Three solves and one more rollout launch (it carries the third solve's sequence), against an eager, untimed
    twin: the same bits, and as many pairs as launches.  Under timing = 1 the stand-alone state-sequence kernel must not have
    run: the rider did the work."""
    lazy, x0 = make("racing", 8, 8192, 1.0, lazy_state_seq=True)
    twin, _ = make("racing", 8, 8192, 1.0)
    lazy.set_option("timing", timing)
    x0 = x0.cuda()
    for _ in range(3):
        a, s = lazy.forward(x0)
        b, t = twin.forward(x0)
    lazy._h.call("mppi_rollout_cost", lazy._stream())
    lazy.join_state_seq()  # (nothing is pending any more)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(torch.as_tensor(s), torch.as_tensor(t))
    _, counts = drain(lazy)
    assert tuple(counts[n] for n in STAGES) == ((0, 4, 0, 0) if timing == 2 else (0, 4, 3, 3)), counts
    if timing == 1:
        assert lazy.stage_times_ms()["state_seq_standalone_launches"] == 0.0
