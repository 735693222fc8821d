"""tests/tail_cases.py reaches what tests/test_gpu_tail_geometry.py claims to run: every shape the solve's tail takes under the
Savitzky-Golay step, every kind of shard list, both sides of the wave-rollout threshold — each property recomputed from the
table's numbers, not read off a name — and the references alone meet the limits the GPU tests hold the kernels to.  No GPU."""
import numpy as np

import tail_cases as tc

f32, f64 = np.float32, np.float64
FLT_MIN = float(np.finfo(f32).tiny)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------------------ constants
def test_constants_are_the_sources():
    """The tables below were chosen for these values: a changed constant fails here instead of silently moving the edges."""
    assert tc.source_constants() == dict(FIN_BLOCK=1024, WAVE_ROLLOUT_MAX_T=63, MPPI_SUMMARY_HEAD=4, SG_MAX_WINDOW=255)
    solve = open(tc.CSRC + "/capi_solve.hip").read()
    for line in tc.ADMISSION_LINES:
        assert line in solve, line
    fin = open(tc.CSRC + "/mppi_finalize.hpp").read()
    for line in ("for (int cidx = threadIdx.x; cidx < row; cidx += FIN_BLOCK) {",
                 "const int dcn = row / T, p = sg.window / 2, n = 2 * T - 1;",
                 "for (int idx = threadIdx.x; idx < n * dcn; idx += FIN_BLOCK) {",
                 "if constexpr (is_racing_model(MODEL) && FAST) {",
                 "const float f = expf((-sm[0]) / lambda - xmax);"):
        assert line in fin, line
    assert "int math_fast = 2;" in open(tc.CSRC + "/mppi_handle.hpp").read() and tc.B1_DEFAULT_MATH == 2
    # the filter only runs when the call stores the warm start
    assert "(store_mean && h->reduce.sg_window > 0) ? h->reduce.sg_window : 0" in solve
    from mppi_playground_amd import _capi

    assert _capi.SUMMARY_HEAD == tc.SUMMARY_HEAD and _capi.MAX_DIM_CONTROL == 4


def test_admission_rule_restated():
    assert tc.sg_admitted(5, 2, 0) and tc.sg_admitted(1, 1, 1) and tc.sg_admitted(1, 1, 3) and not tc.sg_admitted(1, 1, 5)
    assert tc.sg_admitted(2, 1, 7) and not tc.sg_admitted(2, 1, 9)
    assert tc.sg_admitted(64, 1, 255) and not tc.sg_admitted(63, 1, 255) and not tc.sg_admitted(200, 1, 257)
    assert tc.sg_admitted(1024, 1, 3) and not tc.sg_admitted(1025, 1, 3) and not tc.sg_admitted(5, 2, 4)
    # each refusal breaks exactly the rule it is listed for
    broken = []
    for T, dc, w in tc.REFUSALS:
        assert not tc.sg_admitted(T, dc, w)
        broken.append((w % 2 == 0, w > tc.SG_MAX_WINDOW, w // 2 > 2 * T - 1, T * dc > tc.FIN_BLOCK))
    assert broken == [(True, False, False, False), (False, True, False, False), (False, False, True, False),
                      (False, False, False, True)]
    assert tc.REFUSALS[1][2] == 257 and tc.REFUSALS[3][0] * tc.REFUSALS[3][1] == 1025


# ------------------------------------------------------------------------------ the filter table
def test_filter_table_reaches_the_shapes():
    S = tc.FILTER_SHAPES
    assert len(set(S)) == len(S)
    assert all(tc.sg_admitted(*s) for s in S)
    # zero history rows: one float per control is allocated, only windows 1 and 3 exist
    t1 = [s for s in S if tc.history_rows(s[0]) == 0]
    assert {(dc, w) for _, dc, w in t1} == {(1, 1), (1, 3), (2, 1), (2, 3)}
    assert all(tc.history_alloc_floats(T, dc) == dc for T, dc, _ in t1) and not tc.sg_admitted(1, 1, 5)
    # one history row: the slot a'[0] lands in; 7 is the widest window its horizon admits
    t2 = [s for s in S if tc.history_rows(s[0]) == 1]
    assert {dc for _, dc, _ in t2} == {1, 2, 4} and {w for _, _, w in t2} == {3, 7}
    assert all(not tc.sg_admitted(T, dc, 9) for T, dc, _ in t2)
    # window / 2 == 2T - 1: the flip copies the whole sequence — at a small horizon, and together with the cap
    whole = [s for s in S if s[2] // 2 == 2 * s[0] - 1]
    assert (3, 1, 11) in whole and (64, 1, 255) in whole and (2, 1, 7) in whole
    assert any(w == tc.SG_MAX_WINDOW and w // 2 < 2 * T - 1 for T, _, w in S)             # capped by 255 only
    # ordinary shapes: padding shorter than the history, and as long as it (the front flip mirrors every history row)
    assert any(w // 2 < T - 1 for T, _, w in S) and any(1 < T - 1 <= w // 2 < 2 * T - 1 for T, _, w in S)
    # row = FIN_BLOCK at 1, 2 and 4 controls: one thread per column while the staging loop strides
    full = [s for s in S if s[0] * s[1] == tc.FIN_BLOCK]
    assert {dc for _, dc, _ in full} == {1, 2, 4} and all(tc.staging_rounds(T, dc) == 2 for T, dc, _ in full)
    assert max(T * dc for T, dc, _ in S) == tc.FIN_BLOCK
    # the generic handles of 3 and 6 controls
    assert any(dc == 3 for _, dc, _ in S) and any(dc == 6 and T * dc == 1020 and tc.staging_rounds(T, dc) == 2 for T, dc, _ in S)
    # the staging fits the 64 KB the host allows: [row] action, [4 + row] summary, the padded sequence
    for T, dc, w in S:
        assert 4 * (2 * T * dc + tc.SUMMARY_HEAD + (2 * T - 1 + 2 * (w // 2)) * dc) <= 64 * 1024, (T, dc, w)


def test_taps_make_an_indexing_error_visible():
    for T, dc, w in tc.FILTER_SHAPES:
        s, a = tc.taps("savgol", T, dc, w), tc.taps("asymmetric", T, dc, w)
        assert s.dtype == f32 and a.dtype == f32 and s.shape == a.shape == (w,)
        assert np.allclose(s, s[::-1], rtol=0, atol=1e-6 * np.abs(s).max())     # the real coefficients are symmetric ...
        assert abs(float(s.astype(f64).sum()) - 1.0) < 1e-4
        assert len(np.unique(a)) == w and np.all(np.abs(a) <= 1.0)              # ... these have no two entries equal
        if w > 1:
            assert np.all(a[: w // 2] != a[::-1][: w // 2])
        if w > 1 and T > 1:  # (T = 1 pads one sample to a constant sequence: nothing to mirror)
            # a reversed tap index moves the filtered row by far more than rounding
            hist, A = tc.history("random", T, dc), tc.filter_row(T, dc, w, 0)
            d = np.abs(tc.convolve64(hist, A, a) - tc.convolve64(hist, A, a[::-1])).max()
            assert d > 1e-3, (T, dc, w, d)
    assert np.array_equal(tc.taps("asymmetric", 5, 2, 5), tc.taps("asymmetric", 5, 2, 5))
    for T, dc, _ in tc.FILTER_SHAPES:
        assert tc.history("zero", T, dc).shape == tc.history("random", T, dc).shape == (T - 1, dc)
        assert T == 1 or np.all(tc.history("random", T, dc) != 0.0)


def test_host_statement_evaluates_every_filter_shape():
    """pi_mpc._host.sg_filter_sequence is the product's sg_filter="host" path and the yardstick the device is held to bit for
    bit: it evaluates every shape the device admits — T = 1 with a (0, dc) history included — and agrees with an independent
    float64 convolution to 2^-23 * window * max|y| * max|c| (window products and window additions of fp32 rounding each)."""
    from pi_mpc import _host

    for T, dc, w in tc.FILTER_SHAPES:
        for kind in tc.TAP_KINDS:
            c = tc.taps(kind, T, dc, w)
            for hk in tc.HISTORY_KINDS:
                hist = tc.history(hk, T, dc)
                for k in range(tc.FILTER_SOLVES):
                    A = tc.filter_row(T, dc, w, k)
                    got = _host.sg_filter_sequence(hist, A, c)
                    assert got.shape == (T, dc) and got.dtype == f32
                    want = tc.convolve64(hist, A, c)
                    ymax = max(float(np.abs(A).max()), float(np.abs(hist).max()) if hist.size else 0.0)
                    lim = 2.0 ** -23 * w * ymax * float(np.abs(c).max())
                    err = float(np.abs(got.astype(f64) - want).max())
                    assert err <= lim, (T, dc, w, kind, hk, k, err, lim)
                    hist = np.concatenate([hist[1:], got[:1]], axis=0) if T > 1 else hist  # the shift of step 7
                    assert hist.shape == (T - 1, dc)


def test_one_shard_hands_the_tail_its_action():
    A = tc.filter_row(5, 2, 5, 0)
    s = tc.one_shard(A)
    assert s.shape == (1, tc.SUMMARY_HEAD + 10) and s.dtype == f32
    cmin, se, se2, sec, a = tc.combine_fp32(s, 1.0)
    assert np.array_equal(bits(a), bits(A.reshape(-1))) and (cmin, se, se2, sec) == (0.0, 1.0, 1.0, 0.0)


# ------------------------------------------------------------------------------ the shard table
def _factors32(case):
    return np.exp(tc.combine_argument(case.summaries[:, 0], case.lam)).astype(f32)


def test_shard_table_reaches_what_it_claims():
    C = tc.SHARD_CASES
    assert len({c.name for c in C}) == len(C)
    assert {1, 2, 3, 8, 64} <= {c.W - len(c.dead) for c in C} and {1, 2, 3, 8, 64} <= {c.W for c in C}
    equal = dead_at = 0
    positions, near, signs, offset, dense = set(), set(), False, False, False
    for c in C:
        s, f = c.summaries, _factors32(c)
        row = c.T * c.dc
        assert s.shape == (c.W, tc.SUMMARY_HEAD + row) and np.all(np.isfinite(s)) and c.lam > 0
        assert 4 * (2 * row + tc.SUMMARY_HEAD) <= 64 * 1024          # the host's LDS bound admits the row
        live = np.array([g not in c.dead for g in range(c.W)])
        assert np.all(s[:, 1:4] > 0)
        if c.name != "w1_se1":                                      # rows in [1, 3] * se: columns bounded away from zero
            u = s[:, tc.SUMMARY_HEAD:] / s[:, 1:2]
            assert np.all(u[live] >= 1.0 - 1e-6) and np.all(u[live] <= 3.0 + 1e-6)
        # dead shards: the fp32 factor is exactly 0 by a margin of 1e4 lambda, and what they hold is large
        arg = tc.combine_argument(s[:, 0], c.lam)
        for g in c.dead:
            assert f[g] == 0.0 and arg[g] <= -tc.DEAD_GAP and np.all(s[g, 1:] == f32(tc.DEAD_VALUE))
            positions.add("first" if g == 0 else "last" if g == c.W - 1 else "middle")
            dead_at += 1
        assert np.all(f[live] > 0.0)
        if c.exact:
            assert np.all(f[live] == 1.0)
            equal += c.W - len(c.dead) > 1
        srt = np.sort(arg[live])[::-1]
        if len(srt) > 1 and -89.0 < srt[-1] < -86.0:              # the smallest live factor sits at the denormal boundary
            near.add(bool(np.exp(float(srt[-1])) < FLT_MIN))
        m = s[live, 0]
        signs |= bool(m.min() < 0 < m.max())
        offset |= bool(m.min() >= 1.0e6 and m.max() - m.min() > 0.5)
        dense |= bool(c.W >= 8 and 0.5 < -srt[-1] < 5.0 and len(np.unique(m)) == c.W)
    assert equal >= 4 and positions == {"first", "last", "middle"} and dead_at >= 10
    assert near == {True, False}, "one gap on each side of FLT_MIN"
    assert signs and offset and dense
    rows = {c.T * c.dc: c.dc for c in C if c.name.startswith("row")}
    assert set(rows) == {1, 3, 4, 5, 1023, 1024, 1025, 2502} and set(rows.values()) == {1, 3, 6}
    assert [tc.combine_rounds(r) for r in (1023, 1024, 1025, 2502)] == [1, 1, 2, 3]
    assert not tc.sg_admitted(1025, 1, 3) and not tc.sg_admitted(417, 6, 3)      # the last two run without a filter
    assert any(c.W == 64 and c.T * c.dc == 2502 for c in C)
    assert any(c.W == 1 and c.exact and c.summaries[0, 1] == 1.0 and c.summaries[0, 4:].min() < 0 for c in C)


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got, f64) - np.asarray(want, f64)) / np.abs(np.asarray(want, f64))))


def test_fp32_restatement_meets_the_gpu_limit():
    """A chain of W <= 64 multiply-adds on all-positive terms, expf and one quotient cost about (W / 2 + 3) * 2^-24 = 2.1e-6:
    the float64 reference leaves room under the plain 1e-5 for any order of the same sums, so the GPU test needs no band."""
    assert (64 / 2 + 3) * 2.0 ** -24 < 0.25 * tc.TOL
    worst = 0.0
    for c in tc.SHARD_CASES:
        cmin, se, se2, sec, a = tc.combine_reference(c.summaries, c.lam)
        g = tc.combine_fp32(c.summaries, c.lam)
        assert g[0] == cmin == c.summaries[:, 0].min()
        if c.name != "w1_se1":
            assert np.all(a >= 1.0 - 1e-6) and np.all(a <= 3.0 + 1e-6)
        err = max(_rel(g[1], se), _rel(g[2], se2), _rel(g[3], sec), _rel(g[4], a))
        worst = max(worst, err)
        assert err <= tc.TOL, (c.name, err)
        for perm in tc.permutations(c.W - len(c.dead)):
            p = tc.combine_fp32(tc.without_dead(c)[perm], c.lam)
            assert max(_rel(p[1], se), _rel(p[2], se2), _rel(p[3], sec), _rel(p[4], a)) <= tc.TOL, c.name
    assert worst <= 0.5 * tc.TOL, worst


def test_exact_and_dead_cases_are_exact_in_the_references():
    for c in tc.SHARD_CASES:
        if c.dead:  # a factor of exactly 0 leaves no trace, in either evaluation
            a, b = tc.combine_reference(c.summaries, c.lam), tc.combine_reference(tc.without_dead(c), c.lam)
            assert a[:4] == b[:4] and np.array_equal(a[4], b[4]), c.name
            a, b = tc.combine_fp32(c.summaries, c.lam), tc.combine_fp32(tc.without_dead(c), c.lam)
            assert a[:4] == b[:4] and np.array_equal(bits(a[4]), bits(b[4])), c.name
        if c.exact:
            want = tc.combine_exact(c.summaries)
            got = tc.combine_fp32(c.summaries, c.lam)
            assert got[:4] == want[:4] and np.array_equal(bits(got[4]), bits(want[4])), c.name
            ref = tc.combine_reference(c.summaries, c.lam)
            assert (f32(ref[1]), f32(ref[2]), f32(ref[3])) == want[1:4], c.name
    one = tc.shard_case("w1_se1")
    assert np.array_equal(bits(tc.combine_exact(one.summaries)[4]), bits(one.summaries[0, 4:]))
    for W in (2, 3, 8, 64):
        ps = tc.permutations(W)
        assert len(ps) >= 1 and all(sorted(p.tolist()) == list(range(W)) for p in ps) and np.array_equal(ps[0], np.arange(W)[::-1])
    assert tc.permutations(1) == []


# ------------------------------------------------------------------------------ the batch-1 table
def test_batch1_table_reaches_both_rollouts():
    for m in tc.WAVE_ROLLOUT_MODELS:
        Ts = tc.B1_HORIZONS[m]
        assert {1, 2, 3, 62, 63, 64, 65} == set(Ts)
        wave = [T for T in Ts if tc.takes_wave_rollout(m, T, 2)]
        assert max(wave) == tc.WAVE_ROLLOUT_MAX_T == 63 and min(T for T in Ts if T not in wave) == 64
        assert max(wave) + 1 == 64                                   # at T = 63 lane 63 holds row T: every lane is in use
        assert not any(tc.takes_wave_rollout(m, T, 0) for T in Ts)   # library math walks lane-serially at every horizon
    for m in ("nav2d", "pendulum", "cartpole"):
        assert tc.B1_HORIZONS[m] == (1, 2, 15) and not tc.takes_wave_rollout(m, 1, 2)
    assert set(tc.B1_CASES) == {(m, T) for m, Ts in tc.B1_HORIZONS.items() for T in Ts} and len(tc.B1_CASES) == 23
    for m, T in tc.B1_CASES:
        lo, hi = (f32(v) for v in tc.B1_LIMITS[m])
        inside, outside = tc.b1_actions(m, T, "inside"), tc.b1_actions(m, T, "outside")
        assert inside.shape == outside.shape == (T, tc.B1_DC[m]) and inside.dtype == outside.dtype == f32
        assert np.all(inside >= lo) and np.all(inside <= hi)
        assert np.all(outside[0] > hi) and (T == 1 or np.all(outside[-1] < lo))
    from helpers import MODEL_CFG

    for m in ("racing", "nav2d", "pendulum", "cartpole"):
        assert (MODEL_CFG[m]["u_min"], MODEL_CFG[m]["u_max"]) == tc.B1_LIMITS[m]
    import racing_discs_ref as R

    assert (R.U_MIN.tolist(), R.U_MAX.tolist()) == tuple(f32(v).tolist() for v in tc.B1_LIMITS["racing_discs"])
    assert R.CASES["n0"][0](3, None).shape == (3, 0, 4) and set(tc.B1_DISC_TABLES) <= set(R.CASES)
    for m in ("racing", "nav2d", "pendulum", "cartpole"):
        xs = tc.b1_starts(m, tc.b1_base_start(m))
        assert len(xs) == (2 if m in tc.B1_HEADING else 1)
        if m in tc.B1_HEADING:
            j = tc.B1_HEADING[m]
            assert abs(float(xs[0][j])) <= np.pi < abs(float(xs[1][j])) and np.array_equal(np.delete(xs[0], j), np.delete(xs[1], j))
