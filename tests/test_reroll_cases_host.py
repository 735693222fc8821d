"""tests/reroll_cases.py on the host: the table reaches every branch it was written for, the reference it is compared
with stays inside the limit at every horizon of the table, and the host's order of every case is the only one the device
may return.  No GPU."""
import numpy as np
import pytest

import reroll_cases as rc


def _named(pred, noise=("regen",)):
    """Names of the (case, k, noise source) triples whose geometry satisfies `pred`."""
    return [f"{c.name}/k{k}/{s}" for c in rc.CASES for k in c.ks for s in noise if pred(rc.geometry(c.model, c.T, c.N, k, s), c)]


def test_geometry_restated_from_the_table():
    """R, steps per group, whole groups, remainder and TopkLds::pregen from (T, dc, N, k) alone — the formula of
    test_lds_layouts_host.test_topk: R = (T * dc + 3) // 4, pregen = not sorted and regenerated noise and R <= 32."""
    for c in rc.CASES:
        dc = rc.DC[c.model]
        for k in c.ks:
            for s in rc.NOISE_SOURCES:
                g = rc.geometry(c.model, c.T, c.N, k, s)
                row = c.T * dc
                assert g["R"] == (row + 3) // 4 and g["spg"] * dc == 4
                assert g["gfull"] * g["spg"] + g["rem"] == c.T and 0 <= g["rem"] < g["spg"]
                srt, gen = k > 1024, s == "regen"
                assert g["pregen"] == ((not srt) and gen and g["R"] <= 32)
                assert g["launch"] == ("sorted" if srt else "direct" if c.N <= 4096 else "select")
                assert 1 <= k <= c.N


def test_every_branch_is_reached_by_a_named_case():
    models = {c.model for c in rc.CASES}
    assert models == set(rc.MODELS) and len(rc.MODELS) == 9
    for dc in (1, 2):
        of = lambda c: rc.DC[c.model] == dc  # noqa: E731
        assert _named(lambda g, c: of(c) and g["gfull"] == 0), dc                    # the partial group is the row's first
        assert _named(lambda g, c: of(c) and g["gfull"] == 1 and g["rem"] == 0), dc  # one whole group, no look-ahead
        assert _named(lambda g, c: of(c) and g["gfull"] >= 2), dc                    # the look-ahead loop turns over
        for rem in range(4 // dc):
            assert _named(lambda g, c: of(c) and g["rem"] == rem), (dc, rem)
            assert _named(lambda g, c: of(c) and g["rem"] == rem and c.model in rc.MLP), (dc, rem)  # the rolled MLP loop
    # both sides of PREGEN_MAX_R, each model of the pair, and the far side with a partial last group
    for m in rc.BOUNDARY:
        on = _named(lambda g, c: c.model == m and g["R"] == 32 and g["pregen"])
        off = _named(lambda g, c: c.model == m and g["R"] == 33 and not g["pregen"] and g["rem"] != 0)
        assert on and off, m
    assert _named(lambda g, c: not g["pregen"] and g["R"] <= 32, noise=("tiles", "inject"))  # the tiles, short rows
    for launch in ("direct", "select", "sorted"):
        for m, T in rc.LAUNCH_MODELS:
            assert _named(lambda g, c: g["launch"] == launch and c.model == m and c.T == T), (launch, m)
    assert _named(lambda g, c: g["launch"] == "sorted" and c.N not in (1024, 2048))  # padded to a power of two
    for m in rc.MODELS:
        assert _named(lambda g, c: c.model == m and g["split_inside_tile"] and g["ragged_last_tile"]), m
        assert _named(lambda g, c: c.model == m and g["split_inside_tile"] and g["threshold"] // 64 == 2), m
    # k on both sides of a wave of candidates, one candidate, all of them
    assert {1, 64, 65, rc.N_BASE} <= {k for c in rc.CASES for k in c.ks}
    # a start with a heading outside [-pi, pi] for every model that accepts one
    for m in rc.ENTRY_GENERAL:
        xs = rc.starts(m)
        assert len(xs) == 2 and abs(xs[1][rc.HEADING[m]]) > np.pi and abs(xs[0][rc.HEADING[m]]) <= np.pi
    # the redo cases: both horizons, both fast levels, the three models whose fast paths a lane can leave
    assert {(c.model, c.T) for c in rc.REDO_CASES} == {(m, T) for m in ("pendulum", "cartpole", "mjcartpole") for T in (5, 25)}
    assert len(rc.REDO_CASES) == 8 and rc.REDO_MATHS == (1, 2) and all(c.N == 192 for c in rc.REDO_CASES)


@pytest.mark.parametrize("model", rc.MODELS)
def test_reference_moves_less_than_the_limit_under_one_ulp_of_the_actions(model):
    """The anchor's limit is the suite's TOL = 1e-5 of max|S|.  It holds only where the reference itself is that well
    conditioned: at every (model, T) of the table, moving every action by one fp32 ulp must move the oracle's states by less."""
    worst = 0.0
    for T in sorted({c.T for c in rc.CASES if c.model == model}):
        e = rc.ulp_probe(model, T)
        worst = max(worst, e)
        assert e < rc.TOL, (model, T, e)
    print(f"[reroll-host] {model}: one ulp of the actions moves S by at most {worst:.2e} of max|S|")


@pytest.mark.parametrize("case", rc.CASES + rc.REDO_CASES, ids=lambda c: c.name)
def test_host_order_is_the_only_one(case):
    """Costs from the reference on philox_normal noise.  Short horizons have tied costs by nature (a saturated control
    row at T = 1, the cart-pole's two forces, the mountain car's squared distance moving by less than an ulp), so the tests
    row at T = 1, the cart-pole's two forces, nav2d's speed clamped to zero, the mountain car's squared distance moving by
    less than an ulp), so the tests order ties by index: every launch sorts (cost key << 32 | index) words, and the one-row
    direct launch — every N = 200 and N = 192 case — sorts ALL samples' words, which leaves no freedom.  The launches fed
    by the radix select pick among equal keys AT THE CUT in the order their atomics meet them: there the k-th and the
    (k + 1)-th key must differ (order_is_determined), or k = N."""
    redo = isinstance(case, rc.Redo)
    for start in ([case.x0] if redo else range(len(rc.starts(case.model)))):
        h = rc.host_solve(case.name, case.model, case.T, case.N, start)
        assert np.all(np.isfinite(h["costs"])) and np.abs(h["costs"]).max() / h["lam"] <= 32.0
        order, keys = rc.host_order(h["costs"])
        assert np.all(np.diff(keys[order].astype(np.int64)) >= 0)
        for k in case.ks:
            launch = rc.geometry(case.model, case.T, case.N, k)["launch"]
            assert rc.order_is_determined(keys, order, k, launch), (case.name, k)
            if launch == "direct":
                assert case.N <= rc.TOPK_MAX  # one row: block_rank_sort_1024 over every sample's word
            else:
                assert k == case.N or keys[order[k - 1]] < keys[order[k]], (case.name, k)
