"""tests/stats_cases.py reaches what tests/test_gpu_stats_geometry.py claims to run: every launch geometry of the two statistics
kernels, every kind of last chunk, the Brent search's groups and its staging limit, the places of a single cost — and the
float64 references alone meet the limits the GPU tests hold the device searches to, with room to spare.  No GPU."""
import math

import numpy as np

import emul
import stats_cases as sc
from helpers import same_lbps_minimum


def test_constants_are_the_kernels():
    """The geometry functions read the headers; the tables below were chosen for these values."""
    k = sc.header_constants()
    assert k == dict(WAVE=64, BLOCK=256, STATS_BLOCKS=256, STATS_THREADS=1024, STATS_L=32, STATS_COMB_GROUPS=40,
                     BRENT_STAGE_MAX=32, LBPS_GRID_ROUNDS=2)
    text = open(sc.CSRC + "/mppi_search.hpp").read()
    for line in ("constexpr int BRENT_LANES = WAVE;", "float p[BRENT_THREADS / WAVE][4];", "float lam, xmax;", "int go;",
                 "const float cv = i < N ? costs[i] : 3.0e38f;", "static constexpr int K = 8;"):
        assert line in text, line
    assert sc.BRENT_LDS_FIXED == 4 * (1024 // 64) * 4 + 12 + 256


def test_geometry_spot_values():
    assert [sc.one_geometry(N) for N in (1, 256, 257, 65536, 65537, 2097153)] == [(1, 1), (1, 1), (2, 1), (256, 1), (256, 2), (256, 33)]
    assert [sc.multi_geometry(N) for N in (1, 1024, 1025, 262144, 262145, 787209)] == [(1, 1), (1, 1), (2, 1), (256, 1), (256, 2), (256, 4)]
    assert sc.brent_geometry(1) == (1, 1, True) and sc.brent_geometry(16385) == (64, 2, True)
    assert sc.brent_geometry(65536) == (64, 4, True) and sc.brent_geometry(3000001) == (64, 4, False)
    assert sc.brent_staging_pair() == (2097152, 2097153) and sc.brent_staging_pair(64 * 1024) == (15 * 65536, 15 * 65536 + 1)
    assert sc.brent_geometry(15 * 65536 + 1, lds_max=64 * 1024)[2] is False and sc.brent_geometry(15 * 65536, lds_max=64 * 1024)[2] is True


def test_multi_table_covers_the_geometries():
    geo = {N: sc.multi_geometry(N) for N in sc.MULTI_SIZES}
    assert sc.MULTI_SIZES == sorted(set(sc.MULTI_SIZES))
    assert {1, 2, 39, 40, 41, 256} <= {B for B, _ in geo.values()}
    assert {r for _, r in geo.values()} == {1, 2, 3, 4}
    # STATS_COMB_GROUPS row groups: one that has no row, exactly one row each, one with two rows
    assert sc.STATS_COMB_GROUPS - 1 in {B for B, _ in geo.values()} and sc.STATS_COMB_GROUPS + 1 in {B for B, _ in geo.values()}
    alone = [N for N in sc.MULTI_SIZES if sc.block0_alone_in_last_round(N)]
    assert {262145, 524289, 787209} <= set(alone)
    assert 262145 - 262144 == 1 and 524289 - 2 * 262144 == 1                        # ... with one live cost
    assert not sc.block0_alone_in_last_round(262144 + 100 * 1024 + 17)             # a second round that 101 blocks run
    assert any(B > 1 and (N - 1) % 1024 == 0 for N, (B, r) in geo.items() if r == 1)  # a last block with one live cost: 1025
    # the last live chunk: ragged, exactly full, in the first half-wave of its wave (the second all padding) and in the second
    chunks = {N: sc.last_chunk(N) for N in sc.MULTI_SIZES}
    assert chunks[1] == (1, 0) and chunks[31] == (31, 0) and chunks[32] == (32, 0) and chunks[33] == (1, 1)
    assert chunks[63] == (31, 1) and chunks[64] == (32, 1) and chunks[65] == (1, 2) and chunks[1024] == (32, 31)
    assert chunks[2079] == (31, 0) and chunks[262144 + 100 * 1024 + 17] == (17, 0) and chunks[787209] == (9, 24)
    live = {c[0] for c in chunks.values()}
    assert 32 in live and 1 in live and any(1 < v < 32 for v in live)
    assert any(c[1] % 2 == 1 and c[0] < 32 for c in chunks.values()) and any(c[1] % 2 == 0 and c[0] < 32 for c in chunks.values())
    # the chain condition behind the limit: 1e-5 everywhere
    for N in sc.MULTI_SIZES:
        assert sc.chain_multi(N) == 32 * geo[N][1] + 16 <= 167 and sc.limit(sc.chain_multi(N)) == 1e-5, N


def test_one_table_covers_the_geometries():
    geo = {N: sc.one_geometry(N) for N in sc.ONE_SIZES}
    assert sc.ONE_SIZES == sorted(set(sc.ONE_SIZES))
    assert {1, 64, 65, 128, 129, 192, 193, 256} <= {nvb for nvb, _ in geo.values()}
    assert {sc.brent_geometry(N)[1] for N in sc.ONE_SIZES} == {1, 2, 3, 4}
    assert {sc.brent_geometry(N)[0] for N in sc.ONE_SIZES} >= {1, 2, 64}
    # virtual blocks 64 / 65, 128 / 129, 192 / 193: the last block of a Brent group and the first of the next, one live cost in it
    for nvb in (65, 129, 193):
        N = (nvb - 1) * 256 + 1
        assert N in geo and geo[N] == (nvb, 1) and N - 1 in geo and geo[N - 1] == (nvb - 1, 1)
    assert {c for _, c in geo.values()} >= {1, 2, 3, 32, 33}
    staged = {N: sc.brent_geometry(N)[2] for N in sc.ONE_SIZES}
    assert staged[2097152] and not staged[2097153] and geo[2097152] == (256, 32) and geo[2097153] == (256, 33)
    assert (2097152, 2097153) == sc.brent_staging_pair()
    assert geo[65537] == (256, 2) and geo[65791] == (256, 2) and 65791 == 65536 + 255   # a second cost for one thread / for all but one of a block
    for N in sc.ONE_SIZES:
        assert sc.chain_one(N) <= 42 and sc.limit(sc.chain_one(N)) == 1e-5
    assert set(sc.ALL_SIZES) == set(sc.ONE_SIZES) | set(sc.MULTI_SIZES)


def test_positions_reach_the_edges():
    for N in sc.ALL_SIZES:
        p = sc.positions(N)
        B, _ = sc.multi_geometry(N)
        nvb, _ = sc.one_geometry(N)
        assert p == sorted(set(p)) and p[0] == 0 and p[-1] == N - 1 and all(0 <= i < N for i in p) and len(p) <= 16
        for i in (31, 32, 63, 64, 255, 256, 1023, 1024, B * 1024 - 1, B * 1024, nvb * 256 - 1, nvb * 256,
                  (N - 1) // 1024 * 1024, (N - 1) // 256 * 256):
            assert (i in p) == (i < N), (N, i)
    assert 262144 in sc.positions(262145) and 262143 in sc.positions(262145)      # both sides of the end of the first round
    assert 65536 in sc.positions(65537) and 65535 in sc.positions(65537)


def test_cost_vectors_and_temperature_sets():
    c = sc.one_live(1025, [1024])
    assert c.dtype == np.float32 and c[1024] == 2.0 and c[0] == 1000002.0 and float(np.float32(sc.DEAD)) == 1000002.0
    # e is exactly 0 or 1 for every temperature up to 1e3, through either kernel's argument
    for lam in (1e-3, 1.0, 1e3):
        for ref in (sc.reference_one, sc.reference_multi):
            assert ref(c, [lam]).tolist() == [[1.0, 1.0, 2.0, 2.0]]
            assert ref(np.full(77, sc.EQUAL, np.float32), [lam]).tolist() == [[77.0, 77.0, 3.25 * 77, 3.25 * 77]]
    assert sc.extreme_at(5, 3, sc.PEAK).tolist() == [5, 5, 5, 7, 5] and sc.extreme_at(1, 0, sc.PIT).tolist() == [1]
    for name, lams in sc.TEMPERATURE_SETS.items():
        assert lams.dtype == np.float32 and len(set(lams.tolist())) == len(lams) and lams.min() >= 1e-3 and lams.max() <= 1e3 * (1 + 1e-6)
    assert [len(v) for v in sc.TEMPERATURE_SETS.values()] == [32, 32, 1, 31, 32]
    s = sc.SET_SHUFFLED
    assert sorted(s.tolist()) == sc.SET_WIDE.tolist() and np.any(np.diff(s) > 0) and np.any(np.diff(s) < 0)
    assert all(s[j] != sc.SET_WIDE[j] for j in range(32))                          # no column keeps its place
    assert abs(sc.SET_NARROW[0] - 0.01) <= 1e-9 and abs(sc.SET_NARROW[-1] - 10.0) <= 1e-6 and abs(sc.SET_WIDE[-1] - 1e3) <= 1e-4
    assert len(sc.DENSE_KINDS) == 16 and len(set(sc.DENSE_KINDS)) == 16
    for kind in sc.DENSE_KINDS:
        for N in (1, 33, 1025):
            c = sc.dense_costs(N, kind)
            assert c.dtype == np.float32 and c.shape == (N,) and np.all(np.isfinite(c)) and np.array_equal(c, sc.dense_costs(N, kind))


def test_references_on_a_hand_example():
    c = np.array([0.3, 0.7, 0.1, -0.2], np.float32)
    lam = np.float32(0.07)
    q = (-c / lam).astype(np.float32)
    one = sc.reference_one(c, [lam])[0]
    e = np.exp((q - q[3]).astype(np.float32).astype(np.float64))
    assert e[3] == 1.0 and np.allclose(one, [e.sum(), (e * e).sum(), (e * c).sum(), (e * np.abs(c)).sum()], rtol=1e-15, atol=0)
    multi = sc.reference_multi(c, [lam])[0]
    x = ((c[3] - c).astype(np.float32) * (np.float32(1) / lam)).astype(np.float32)
    e2 = np.exp(x.astype(np.float64))
    assert np.allclose(multi, [e2.sum(), (e2 * e2).sum(), (e2 * c).sum(), (e2 * np.abs(c)).sum()], rtol=1e-15, atol=0)
    assert not np.array_equal(e, e2) and np.allclose(e, e2, rtol=1e-5)             # the two arguments round differently
    assert sc.sums_error(one[:3], one) == 0.0
    assert abs(sc.sums_error(one[:3] * [1.0, 1.0 + 1e-6, 1.0], one) - 1e-6) < 1e-9
    # sum e*c is measured against sum e*|c|: costs of both signs that nearly cancel do not blow the error up
    assert abs(sc.sums_error([one[0], one[1], one[2] + 1e-6 * one[3]], one) - 1e-6) < 1e-9
    assert abs(sc.sums_error([one[0], one[1], one[2] + 3e-6 * one[3]], one, floor=2e-6 * one[3]) - 1e-6) < 1e-9
    assert sc.sums_error([one[0], one[1], one[2] + 1e-6 * one[3]], one, floor=2e-6 * one[3]) == 0.0
    assert sc.underflow_floor(np.array([1.0, -2.0, 0.0], np.float32)) == 6 * 2.0 ** -149
    assert sc.ulp32(1.0, 1.0) == 0 and sc.ulp32(1.0, np.nextafter(np.float32(1), np.float32(2))) == 1.0
    assert sc.ulp32(-3.0, np.nextafter(np.float32(-3), np.float32(0))) <= 1.0 and sc.ulp32(0.0, 1e-3) > 1e6
    assert sc.softplus32(0.0) == np.float32(math.log(2.0)) and sc.grid_point(0.01, 10.0, 0) == 0.01 and sc.grid_point(0.01, 10.0, 31) == 10.0
    assert sc.lbps_objective(1.0, 3.0, 2.0, 2.0, 4.0, 0.5) == 2.0 + 2.0 / math.sqrt(2.0)


def _essps_case(args):
    N, kind = args
    c = sc.dense_costs(N, kind)
    out = []
    for target in sc.essps_targets(N):
        end = sc.essps_end_point(c, target, sc.LAM_MIN, sc.LAM_MAX)
        lam = emul.essps(c, target, sc.LAM_MIN, sc.LAM_MAX, grid_argument=True)
        off = abs(sc.ess64(c, lam) - target) / target
        ends = [abs(sc.ess64(c, b) - target) / target for b in (sc.LAM_MIN, sc.LAM_MAX)]
        out.append((N, kind, target, end, lam, off, min(ends)))
    return out


def test_essps_reference_meets_its_band_alone():
    """On every ESSPS case of the GPU file the search over float64 sums (of the argument the device chain forms) leaves
    |ESS64 - target| <= 2e-5 target or sits on the end point float64 decides — and no end-point decision is so close that fp32
    sums could fall on the other side of it.  (Over mppi_softmax_stats's argument the same search is 1.2e-2 off at N = 33 with
    the offset of 1e6: its quotients -c / lambda carry 2^-24 * 1e6 / lambda of rounding each.)"""
    emul.search_lib()
    worst = 0.0
    for rows in sc.pmap(_essps_case, [(N, k) for N in sc.SEARCH_SIZES for k in sc.ESSPS_SHAPES]):
        for N, kind, target, end, lam, off, margin in rows:
            if end is not None:
                assert lam == end, (N, kind, target, lam, end)
            else:
                assert sc.LAM_MIN < lam < sc.LAM_MAX and off <= sc.ESS_BAND_REFERENCE, (N, kind, target, lam, off)
                worst = max(worst, off)
            assert margin == 0.0 or margin > 10 * sc.ESS_BAND, (N, kind, target, margin)
    print(f"[stats] essps reference alone: largest |ESS64 - target| / target {worst:.3e} (limit {sc.ESS_BAND_REFERENCE:.0e})")


def lbps_vectors(N):
    """(label, costs) of the LBPS grid search's cases at N: the dense Brent kinds and one maximum-at-p vector (the float64 sums
    of the others are the same sums in another order) and one dense vector whose maximum is a single raised cost (likewise)."""
    return [(k, sc.dense_costs(N, k)) for k in sc.DENSE_KINDS[:sc.BRENT_KINDS]] + [("max_at_0", sc.extreme_at(N, 0, sc.PEAK)),
                                                                                   ("raised_at_0", sc.raised_max_at(N, 0))]


def _lbps_case(args):
    N, label, c, delta = args
    return N, label, delta, c, emul.lbps_grid(c, delta, sc.LAM_MIN, sc.LAM_MAX), emul.lbps(c, delta, sc.LAM_MIN, sc.LAM_MAX)[0]


def test_lbps_grid_reference_meets_its_band_alone():
    """On every LBPS case of the GPU file the grid search and the Brent search over float64 sums find the same minimum
    (same_lbps_minimum).  Where the objective is a plateau — equal costs, two cost values, 5.0 everywhere and 7.0 once: below
    some temperature every weight is 0 or 1 in float64 and the objective constant — every point of it is a minimiser, the grid
    search returns its first and Brent an inner one; there the two must sit on the same plateau instead: the float64 objective
    at both and between them is one value.  Only those three kinds may take that branch."""
    emul.search_lib()
    jobs = [(N, label, c, delta) for N in sc.SEARCH_SIZES for label, c in lbps_vectors(N) for delta in sc.LBPS_DELTAS]
    plateaus = []
    for N, label, delta, c, lam_grid, lam_brent in sc.pmap(_lbps_case, jobs):
        assert sc.LAM_MIN <= lam_grid <= sc.LAM_MAX
        if same_lbps_minimum(c, lam_grid, lam_brent, delta=delta):
            continue
        assert sc.on_one_plateau(c, lam_grid, lam_brent, delta), (N, label, delta, lam_grid, lam_brent)
        assert label.startswith(sc.PLATEAU_KINDS), (N, label, delta, lam_grid, lam_brent)
        plateaus.append((N, label, delta))
    print(f"[stats] lbps reference alone: {len(jobs) - len(plateaus)} of {len(jobs)} cases have a point minimum, plateaus: {plateaus}")
    assert len(plateaus) <= len(jobs) // 4


def test_lbps_grid_step_and_mpo_step_entries():
    """The two entries added for the GPU twins are the functions the kernels call: a whole grid search stepped from outside
    equals search_lbps_grid, one MPO step from given statistics equals search_mpo's."""
    c = sc.dense_costs(1000, "brent2")
    cmin, cmax = float(c.min()), float(c.max())
    lo, hi = sc.LAM_MIN, sc.LAM_MAX
    for r in range(sc.LBPS_GRID_ROUNDS):
        grid = [sc.grid_point(lo, hi, j) for j in range(32)]
        sums = sc.reference_multi(c, np.asarray(grid, np.float32))
        obj = [sc.lbps_objective(cmin, cmax, s[0], s[1], s[2], 0.01) for s in sums]
        lo, hi, lam = emul.lbps_grid_step(grid, obj, r == sc.LBPS_GRID_ROUNDS - 1)
    want = emul.lbps_grid(c, 0.01, sc.LAM_MIN, sc.LAM_MAX)
    assert abs(lam - want) <= 1e-9 * want, (lam, want)       # (the sums here are numpy's, in another order)
    rows = np.stack([sc.dense_costs(1000, "brent0"), sc.dense_costs(1000, "brent1")])
    want = emul.mpo(rows, 1.0, 0.1, 0.2)
    state = np.array([0.0, 0.0, 0.0, 0.0])
    for k in range(2):
        T = sc.softplus32(state[0])
        s = sc.reference_one(rows[k], [T])[0]
        state, lam = emul.mpo_step_stats(state, 0.1, 0.2, [rows[k].min(), rows[k].max(), s[0], s[1], s[2]])
        assert state[3] == k + 1 and abs(lam - want[k]) <= 1e-6 * want[k], (k, lam, want[k])
