"""tests/fused_cases.py reaches what tests/test_gpu_fused_geometry.py claims to run: every block geometry of the single-launch
solve, every row rounding, the winners' places, and a tolerance that follows from the chain lengths.  No GPU."""
import math
import os
import re

import numpy as np

import fused_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _size_geometries():
    return [(N,) + fc.geometry(N, mode=fc.fused_mode(N)) for N in fc.SIZE_NS]


def test_constants_are_the_kernels():
    """The restated constants are the ones mppi_fused.hpp and capi_solve.hip define."""
    hpp = open(os.path.join(ROOT, "mppi_playground_amd", "csrc", "mppi_fused.hpp")).read()
    hip = open(os.path.join(ROOT, "mppi_playground_amd", "csrc", "capi_solve.hip")).read()
    for name, text in (("FUSED_BLOCK", hpp), ("FUSED_MAX_BLOCKS", hpp), ("FUSED_MAX_ROW", hpp), ("FUSED_SMALL_BLOCKS", hpp), ("KG", hpp)):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == getattr(fc, name), name
    assert "constexpr int FX_CELLS = FUSED_MAX_ROW + 8;" in hpp
    assert "FUSED_AUTO_MAX_SAMPLES = %d;" % fc.AUTO_MAX_SAMPLES in hip and "FUSED_AUTO_MAX_SAMPLES_SEARCH = %d;" % fc.AUTO_MAX_SAMPLES_SEARCH in hip
    assert (fc.RPARTS, fc.SPARTS, fc.KS) == (3, 5, 11)
    for cond in ("KS * RPARTS >= FUSED_SMALL_BLOCKS", "KS * SPARTS >= FUSED_SMALL_BLOCKS", "FUSED_MAX_BLOCKS <= FUSED_BLOCK / 2",
                 "FUSED_MAX_ROW + MPPI_SUMMARY_HEAD <= FX_CELLS", "STATS_L * 3 + 2 <= FX_CELLS"):
        assert "static_assert(" + cond in hpp, cond


def test_geometry_spot_values():
    want = {1: (1, 64), 64: (1, 64), 65: (2, 64), 2048: (32, 64), 2049: (17, 128), 4096: (32, 128), 1000: (16, 64)}
    for N, g in want.items():
        assert fc.geometry(N) == g, N
    want2 = {4097: (65, 64), 6145: (97, 64), 16384: (256, 64), 16385: (129, 128), 130561: (256, 512), 131072: (256, 512)}
    for N, g in want2.items():
        assert fc.geometry(N, mode=2) == g, N
        assert fc.geometry(N) is None                          # "fused_solve" = 1 with a fixed temperature stops at 4096
    assert fc.geometry(16384, search=True) == (256, 64) and fc.geometry(16385, search=True) is None
    assert fc.geometry(4097, search=True) == (65, 64)
    assert fc.geometry(131073, mode=2) is None and fc.geometry(1000, mode=0) is None
    assert fc.geometry(1000, row=128) == (16, 64) and fc.geometry(1000, row=129) is None
    # fewer compute units: fewer, larger blocks, and a smaller largest problem
    assert fc.geometry(16384, cu=64, mode=2) == (64, 256) and fc.geometry(512 * 64 + 1, cu=64, mode=2) is None
    assert fc.geometry(262144, mode=2) is None                 # the size the old parity case named


def test_size_table_covers_the_block_geometries():
    geo = _size_geometries()
    assert [N for N, _, _ in geo] == sorted(set(fc.SIZE_NS))
    assert {spb for _, _, spb in geo} == set(range(64, 513, 64))
    assert {1, 2, 17, 32, 65, 97, 129, 256} <= {G for _, G, _ in geo}
    for N, G, spb in geo:
        assert (G - 1) * spb < N <= G * spb and spb <= fc.FUSED_BLOCK and G <= fc.FUSED_MAX_BLOCKS
    last = {N: N - (G - 1) * spb for N, G, spb in geo}
    one_lane = [N for N, G, spb in geo if G > 1 and last[N] == 1]
    assert {65, 2049, 130561} <= set(one_lane)
    assert any(spb - last[N] >= 64 for N, G, spb in geo if G > 1)             # a last block with empty waves
    assert 512 - last[130561] >= 7 * 64                                       # seven of them
    # both sides of the switch between the own-minimum path and the minimum hop, and a second pass of the hop path's loops
    small = [G for N, G, _ in geo if G <= fc.FUSED_SMALL_BLOCKS]
    assert max(small) == fc.FUSED_SMALL_BLOCKS and min(G for N, G, _ in geo if G > fc.FUSED_SMALL_BLOCKS) == 65
    assert fc.geometry(4096) == (32, 128) and fc.geometry(4097, mode=2)[0] > fc.FUSED_SMALL_BLOCKS
    assert any(G > fc.KG * fc.RPARTS for _, G, _ in geo) and any(G > fc.KG * fc.SPARTS for _, G, _ in geo)
    assert max(N for N, _, _ in geo) == fc.FUSED_BLOCK * fc.FUSED_MAX_BLOCKS
    # the exploration split falls inside a block for some entries of both paths
    inside = [N for N in fc.SIZE_NS if fc.split_inside_a_block(N)]
    assert any(fc.geometry(N, mode=2)[0] <= 32 for N in inside) and any(fc.geometry(N, mode=2)[0] > 32 for N in inside)
    for N in inside:
        G, spb = fc.geometry(N, mode=2)
        k = fc.inherit_count(N)
        assert (k - 1) // spb == k // spb                                      # samples k - 1 and k share a block


def test_row_table_covers_every_rounding():
    assert fc.geometry(fc.ROW_TABLE_N) == (16, 64)
    seen = {}
    for model, T in fc.ROW_TABLE:
        dc = fc.DIM_CONTROL[model]
        R, RP = fc.row_shape(T, dc)
        assert R == math.ceil(T * dc / 4) and RP >= R and RP & (RP - 1) == 0 and (RP == 1 or RP // 2 < R)
        assert fc.geometry(fc.ROW_TABLE_N, row=T * dc) == (16, 64)
        seen.setdefault(RP, set()).add(R)
    assert set(seen) == {1, 2, 4, 8, 16, 32}
    for RP in (4, 8, 16, 32):
        assert RP in seen[RP] and any(R != RP for R in seen[RP]), RP           # R a power of two and not
    rows = {T * fc.DIM_CONTROL[m] for m, T in fc.ROW_TABLE}
    assert fc.FUSED_MAX_ROW in rows and 1 in rows and any(r % 4 for r in rows)  # the widest row, the narrowest, ragged last groups
    assert {"pendulum", "nav2d"} == {m for m, _ in fc.ROW_TABLE}
    m, T = fc.ROW_TOO_WIDE
    assert fc.geometry(fc.ROW_TABLE_N, row=T * fc.DIM_CONTROL[m]) is None


def test_targets_reach_the_edges():
    blocks_small, blocks_hop = set(), set()
    for N, G, spb in _size_geometries():
        t = fc.targets(N, G, spb)
        assert t == sorted(set(t)) and t[0] == 0 and t[-1] == N - 1 and len(t) <= 12
        blk = {i // spb for i in t}
        assert 0 in blk and G - 1 in blk
        if N >= 64:
            assert any(i % 64 == 63 for i in t) and any(i % 64 == 0 for i in t)
        if G >= 2:
            assert (G - 1) * spb in t and (G - 1) * spb - 1 in t               # first lane of the last block, last lane of the one before
        if N > spb:
            assert spb - 1 in t and spb in t
        (blocks_small if G <= fc.FUSED_SMALL_BLOCKS else blocks_hop).update((G, b) for b in blk)
        edge = (10, 11, 30, 31) if G <= fc.FUSED_SMALL_BLOCKS else (95, 96, 97, 255)
        for b in edge:
            assert (b in blk) == (b < G), (N, b)
    # block 31 of the largest own-minimum grid is the last cell of the last thread: KS * RPARTS = 33 > 31 >= (KS - 1) * RPARTS
    assert (32, 31) in blocks_small and (32, 30) in blocks_small and (fc.KS - 1) * fc.RPARTS <= 31 < fc.KS * fc.RPARTS
    assert {(256, 95), (256, 96), (256, 97), (256, 255)} <= blocks_hop and fc.KG * fc.RPARTS == 96


def test_reference_on_a_hand_example():
    U = np.array([[[1.0], [2.0]], [[3.0], [1.5]], [[2.5], [2.5]]], np.float32)  # [3 samples][T = 2][dc = 1]
    costs = np.array([2.0, 1.0, 3.0], np.float32)
    w1, w2 = math.exp(-1.0), math.exp(-2.0)
    # one block of 64, and more than 32 blocks (any spb): the argument is c_min - c
    for G, spb in ((1, 64), (65, 64)):
        cmin, se, se2, sec, A = fc.reference(U, costs, 1.0, G, spb)
        assert cmin == 1.0 and se == 1.0 + w1 + w2 and se2 == 1.0 + w1 * w1 + w2 * w2 and sec == 2.0 * w1 + 1.0 + 3.0 * w2
        assert np.allclose(A, [w1 * 1.0 + 3.0 + w2 * 2.5, w1 * 2.0 + 1.5 + w2 * 2.5], rtol=1e-15, atol=0)
    # own minima: "blocks" of one sample each (spb = 1 is no launch geometry, but it is the formula): every sample has weight
    # exp(0) in its block and the block's factor carries all of it
    cmin, se, se2, sec, A = fc.reference(U, costs, 1.0, 3, 1)
    assert cmin == 1.0 and se == w1 + 1.0 + w2 and sec == 2.0 * w1 + 1.0 + 3.0 * w2
    # blocks {0, 1} and {2}, the minimum in the second: sample 1 is weighted relative to sample 0, its block's reference, and the
    # block's factor brings it to the minimum; where the quotients round, the two forms differ in the last bits of the argument
    c = np.array([0.3, 0.7, 0.1], np.float32)
    lam = np.float32(0.07)
    q = (-c / lam).astype(np.float32)
    own = fc.weights(c, lam, 2, 2)
    hop = fc.weights(c, lam, 2, 2, search=True)
    assert np.array_equal(hop, np.exp((q - q[2]).astype(np.float32).astype(np.float64))) and hop[2] == 1.0
    f0 = math.exp(float(np.float32(q[0] - q[2])))
    assert own[2] == 1.0 and own[0] == f0 == hop[0]
    assert own[1] == math.exp(float(np.float32(q[1] - q[0]))) * f0 and abs(own[1] - hop[1]) <= 1e-5 * hop[1]
    assert np.array_equal(fc.weights(c, lam, 33, 2), hop)
    # a sample of weight 0 is left out even with an infinite cost
    cmin, se, se2, sec, A = fc.reference(U, np.array([1.0, np.inf, 1.0], np.float32), 1.0, 1, 64)
    assert (se, se2, sec) == (2.0, 2.0, 2.0) and np.array_equal(A, [3.5, 4.5])
    sc, S = fc.scales(-U, np.array([-2.0, -1.0, -3.0], np.float32), np.array([1.0, 0.0, 0.5]))
    assert sc == 2.0 + 1.5 and np.array_equal(S, [1.0 + 1.25, 2.0 + 1.25])


def test_chain_lengths_keep_the_limit():
    worst = 0
    for N, G, spb in _size_geometries():
        worst = max(worst, fc.chain(G, spb, fc.row_shape(fc.SIZE_T, 1)[0]))
    for model, T in fc.ROW_TABLE:
        worst = max(worst, fc.chain(16, 64, fc.row_shape(T, fc.DIM_CONTROL[model])[0]))
    assert worst * 2.0 ** -24 <= 2e-5
    # hand values: R = 2 at G = 256, spb = 512: 2 samples per thread, 4 slices, 64 groups, ceil(256 / 3) blocks, 3 row groups
    assert fc.chain(256, 512, 2) == 2 + 4 + 64 + 86 + 3
    assert fc.chain(32, 128, 2) == 1 + 4 + 64 + 11 + 3 and fc.chain(16, 64, 32) == 4 + 4 + 4 + 6 + 3
    assert fc.chain(16, 64, 1) == 1 + 4 + 128 + 6 + 3
    assert fc.limit(256, 512, 2) == 1e-5 and fc.limit(16, 64, 1) == 1e-5
