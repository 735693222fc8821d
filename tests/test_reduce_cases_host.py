"""tests/reduce_cases.py reaches what tests/test_gpu_reduce_geometry.py claims to run: every loop position of the reductions'
tile loop, every group count per wave, every published-row count around the fold threshold.  No GPU."""
import math

import numpy as np

import reduce_cases as rc
from test_gpu_covariance import weights64


def _sparse_cases():
    """(geometry name, reduce_blocks option, N, B, label, live sample indices) of every 0 / 1 cost vector the GPU file runs."""
    for name, N, rb in rc.SAMPLE_AXIS:
        B = rc.blocks(N, rb)
        for label, costs, lam, live in rc.sample_axis_costs(name):
            if live is not None:
                yield name, rb, N, B, label, live


def test_geometry_restatement():
    assert rc.blocks(1) == 1 and rc.blocks(2 ** 20) == 512 and rc.blocks(2 ** 20, 4096) == 2048 and rc.blocks(613) == 3
    assert rc.blocks(5000, 1) == 1 and rc.blocks(256, 512) == 1 and rc.blocks(257, 512) == 2
    for B in (1, 2, 3, 512, 2048):
        t = np.arange(3 * 32 * B + 5)
        rnd, q, blk, wav = rc.coords(t, B)
        assert np.array_equal(rc.tile_of(rnd, q, blk, wav, B), t)
        assert q.max() == 7 and blk.max() == B - 1 and wav.max() == 3 and rnd.max() == 3
    # the kernel's own walk: block b, wave w, round r, slot q -> tile (4b + 32Br) + w + q * 4B
    B = 3
    for b in range(B):
        for r in range(2):
            base0 = 4 * b + r * 4 * B * 8
            for w in range(4):
                for q in range(8):
                    assert rc.coords(base0 + w + q * 4 * B, B) == (r, q, b, w)
    assert rc.coords(16384, 512) == (1, 0, 0, 0)


def test_sample_axis_table_covers_the_tile_loop():
    qs, waves, rounds, Bs = set(), set(), set(), set()
    late_only = ragged_last = g8_round1 = both_ends = False
    for name, rb, N, B, label, live in _sparse_cases():
        Bs.add(B)
        tiles = np.unique(live // 64)
        rnd, q, blk, wav = rc.coords(tiles, B)
        qs |= set(q.tolist())
        waves |= set(wav.tolist())
        rounds |= set(rnd.tolist())
        for r, b in zip(rnd, blk):  # a live tile in a later round whose block had nothing live before it
            if r >= 1 and not np.any((blk == b) & (rnd < r)):
                late_only = True
        if N % 64 and (N - 1) // 64 in tiles:
            ragged_last = True
        if name == "G8" and rb is None and 1 in rnd:
            g8_round1 = True
        if label == "sparse":
            assert 0 in live and N - 1 in live
            lanes = {t: set((live[live // 64 == t] % 64).tolist()) for t in tiles}
            both_ends |= any({0, 63} <= s for s in lanes.values())
            # the first and last tile of every round that exists, every q in its first and last block, every wave
            arnd, aq, ablk, awav = rc.coords(np.arange(rc.ntiles(N)), B)
            for r in np.unique(arnd):
                mine = np.nonzero(arnd == r)[0]
                assert mine[0] in tiles and mine[-1] in tiles
            for qq in np.unique(aq):
                have = ablk[aq == qq]
                got = blk[q == qq]
                assert have.min() in got and have.max() in got
            assert set(wav.tolist()) == set(awav.tolist())
        assert len(live) <= rc.MAX_LIVE
    assert qs == set(range(8)) and waves == set(range(4)) and {0, 1, 2} <= rounds
    assert late_only and ragged_last and g8_round1 and both_ends
    assert {1, 2, 3, 512, 2048} <= Bs
    assert rc.blocks(*rc.geometry("G8")[1:]) == 512 and rc.ntiles(rc.geometry("G8")[1]) > 32 * 512  # the default grid's second round
    names = [g[0] for g in rc.SAMPLE_AXIS]
    assert rc.EXPLORE_SPLIT in names and set(rc.VARIANCE_GEOMETRIES) <= set(names) and rc.FOLD_GEOMETRY in names
    N = rc.geometry(rc.EXPLORE_SPLIT)[1]
    assert (3 * N // 4) % 64 != 0  # the exploration split falls inside a tile


def test_sample_axis_table_keeps_the_tolerance_condition():
    """A lane's sequential fp32 chain is N / (64 B) tiles: at most 80 (80 * 2^-24 = 4.8e-6 < 1e-5)."""
    for name, N, rb in rc.SAMPLE_AXIS:
        assert N / (64.0 * rc.blocks(N, rb)) <= 80.0, name
    T, dc, N = rc.CHAINS2_BY_RULE
    assert N / (64.0 * rc.blocks(N)) <= 80.0 and rc.ROW_TABLE_N / (64.0 * rc.blocks(rc.ROW_TABLE_N)) <= 80.0


def test_one_per_block_publishes_the_rows_it_names():
    _, N, rb = rc.geometry(rc.FOLD_GEOMETRY)
    B = rc.blocks(N, rb)
    assert B == 512
    counts = set()
    for label, costs, live in rc.fold_costs():
        blk = rc.coords(live // 64, B)[2]
        assert len(np.unique(blk)) == len(live)  # one sample per block, distinct blocks
        counts.add(len(live))
        if label.endswith("first"):
            assert blk.max() == len(live) - 1
        if label.endswith("last"):
            assert blk.min() == B - len(live)
    assert counts == set(rc.FOLD_LIVE_ROWS)
    assert {rc.FOLD_IN_FINALIZE_MAX_ROWS - 1, rc.FOLD_IN_FINALIZE_MAX_ROWS, rc.FOLD_IN_FINALIZE_MAX_ROWS + 1} <= counts


def test_row_table_covers_every_group_count():
    pairs, chunks, ragged, wide = set(), set(), set(), 0
    for R, T, dc, is_wide in rc.row_table():
        R2, nch, per, rag = rc.row_shape(T, dc)
        assert R2 == R == math.ceil(T * dc / 4) and len(per) == nch
        assert sum(4 * f + r for f, r in per) == R
        pairs |= set(per)
        chunks.add(nch)
        ragged.add(rag)
        wide += is_wide
        assert is_wide == (dc not in (1, 2, 4))
    possible = {(ng // 4, ng % 4) for ng in range(1, 33)}
    assert possible == {(f, r) for f in range(9) for r in range(4)} - {(0, 0), (8, 1), (8, 2), (8, 3)}
    assert pairs == possible
    assert chunks == {1, 2, 3} and ragged == {False, True} and wide == 3
    dc1 = {T for R, T, dc, w in rc.row_table() if dc == 1}
    assert all(4 * R in dc1 and 4 * R - 1 in dc1 for R in list(range(1, 35)) + [40, 63, 64, 65])
    assert rc.row_shape(87, 1)[0] == 22 and rc.row_shape(50, 2)[0] == 25
    # the host's own rule picks CHAINS = 2 beyond 2 * 256 blocks x chunks (capi_solve.hip: `blocks * nchunks <= 2 * cu_count`)
    T, dc, N = rc.CHAINS2_BY_RULE
    assert rc.blocks(N) == 300 and rc.row_shape(T, dc)[1] == 2 and rc.blocks(N) * rc.row_shape(T, dc)[1] > 2 * 256


def test_reference_on_a_hand_example():
    U = np.array([[[1.0], [2.0]], [[3.0], [1.5]], [[2.5], [2.5]]], np.float32)  # [3 samples][T = 2][dc = 1]
    costs = np.array([1.0, 2.0, np.inf], np.float32)
    se, se2, sec, A = rc.reference(U, costs, 1.0)
    w = math.exp(-1.0)
    assert se == 1.0 + w and se2 == 1.0 + w * w and sec == 1.0 + 2.0 * w
    assert np.array_equal(A, np.array([1.0 + 3.0 * w, 2.0 + 1.5 * w]))
    se, se2, sec, A = rc.reference(U, np.array([5.0, 3.0, 3.0], np.float32), 0.5)
    w = math.exp(-4.0)
    assert np.allclose([se, se2, sec], [2.0 + w, 2.0 + w * w, 6.0 + 5.0 * w], rtol=1e-15)
    assert np.allclose(A, [w * 1.0 + 3.0 + 2.5, w * 2.0 + 1.5 + 2.5], rtol=1e-15)


def test_sparse_costs_give_exact_weights():
    n = 0
    for name, rb, N, B, label, live in _sparse_cases():
        costs = dict((c[0], c[1]) for c in rc.sample_axis_costs(name))[label]
        e, ess = weights64(costs, 1.0)
        assert set(np.unique(e).tolist()) <= {0.0, 1.0}
        assert np.array_equal(np.nonzero(e == 1.0)[0], live) and ess == len(live)
        assert costs.min() == np.float32(rc.LIVE_COST)
        n += 1
    assert n >= 3 * len(rc.SAMPLE_AXIS) - 8
    for label, costs, live in rc.fold_costs():
        e, _ = weights64(costs, 1.0)
        assert np.array_equal(np.nonzero(e)[0], live) and set(np.unique(e).tolist()) <= {0.0, 1.0}


def test_dense_costs_are_what_they_say():
    rng = np.random.default_rng(5)
    c, lam = rc.dense_costs(30000, "uniform", rng)
    assert abs(weights64(c, lam)[1] / 30000 - 1.0 / 3.0) < 0.02
    c, lam = rc.dense_costs(1000, "equal", rng)
    assert weights64(c, lam)[1] == 1000.0
    c, lam = rc.dense_costs(1000, "offset", rng)
    assert c.min() >= 1.0e6 and c.max() <= 1.0e6 + 1.0 and len(np.unique(c)) > 8
    c, lam = rc.dense_costs(5000, "inf", rng)
    assert 0.15 < np.mean(np.isinf(c)) < 0.25
    assert np.isfinite(rc.dense_costs(1, "inf", rng)[0][0])
