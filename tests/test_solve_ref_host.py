"""tests/solve_ref.py without a GPU: the composite restatement is anchored to the single-feature references it is composed of,
every feature-pair case of tests/test_gpu_feature_pairs.py is shown to SEE the mistakes that pair could hide, and every case
keeps its boundary samples within the cap.  The noise is numpy's (solve_ref.numpy_normals) through the restated draw.

(a) anchoring     with exactly one feature on, solve_ref.tick returns that feature's existing reference to the last bit.
(b) sensitivity   per pair and per feature of the pair: a deliberately wrong restatement (the feature dropped, or a misreading
                  from solve_ref.WRONG where the pair admits it) moves a quantity the GPU test compares by at least ten times
                  the limit the GPU test holds that quantity to.
(c) the cap       boundary samples per tick, from the float64 and from the float32 closed loop: at most max(1, N // 100).
"""
import numpy as np
import pytest

import action_cost_ref as acref
import emul
import mlp_ref as ML
import particle_cases as pc
import racing_discs_ref as RD
import soft_discs_ref as SD
import solve_ref as sr
from helpers import oracle_problem
from pi_mpc import _host
from test_covariance_host import numpy_step
from test_gpu_action_cost import softmax_action
from test_gpu_colored_noise import colored
from test_gpu_covariance import restate, weights64

f32, f64 = np.float32, np.float64
NP = sr.numpy_normals
IDS = [sr.pair_id(p) for p in sr.PAIRS]


def bits64(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


def same64(name, got, want):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = int(np.sum(bits64(got) != bits64(want)))
    assert bad == 0, f"{name}: {bad} of {got.size} values differ"


def one_feature(feature, family):
    """A problem of `family` with `feature` alone switched on (the shapes of a pair that holds it)"""
    pair = next(p for p in sr.PAIRS if (feature is None or feature in p) and sr.rotation()[p][0] == family)
    model, x0 = sr.host_model(family)
    return sr.Problem(pair, model, x0, {feature} if feature else set())


def first_tick(pb, dtype=f64):
    carry = pb.carry0()
    eps = sr.eps_for(pb, carry, 1, normals=NP)
    return carry, eps, sr.tick(pb, carry, eps, dtype)


# ---------------------------------------------------------------------------------------------- the table itself
def test_rotation_covers():
    rot = sr.rotation()
    assert len(sr.PAIRS) == 28 and set(rot) == set(sr.PAIRS)
    for f in sr.FEATURES:
        assert {rot[p][0] for p in sr.PAIRS if f in p} == set(sr.FAMILIES), f
    assert {rot[p][1] for p in sr.PAIRS if "TL" in p} == set(sr.RULES)
    assert all(rot[p][1] is None for p in sr.PAIRS if "TL" not in p)
    shapes = {(sr.host_problem(p).N, sr.host_problem(p).T, sr.host_problem(p).dc) for p in sr.PAIRS}
    assert shapes == {(320, 5, 2), (320, 7, 1), (200, 5, 2), (200, 7, 1)}
    assert any(len(sr.host_problem(p).sg) == sr.widest_window(sr.host_problem(p).T) for p in sr.PAIRS if "SG" in p)
    assert sr.host_model("nav_soft")[0].table.shape[1] == 8 and sr.SOFTNESS[0] > 1 and sr.SOFTNESS[1] > 0
    assert {sr.host_problem(p).risk for p in sr.PAIRS if "PR" in p} == {("cvar", 2), ("worst", 1)} and sr.PARTICLES == 3


# ---------------------------------------------------------------------------------------------- (a) anchoring
@pytest.mark.parametrize("family", ["pendulum", "cartpole"])
def test_anchor_plain_tick_is_the_oracle_and_the_float64_softmax(family):
    pb = one_feature(None, family)
    carry, eps, o = first_tick(pb)
    P = oracle_problem(family, pb.N, pb.T)
    r = P.rollout_cost(pb.x0, carry["mean"], eps, want_U=True)
    assert o["U"].dtype == f32 and np.array_equal(o["U"], r["U"])
    same64("costs", o["costs"], r["costs"])
    same64("action", o["action"], softmax_action(r["costs"], pb.lams[0], r["U"]))
    e, ess = weights64(r["costs"], pb.lams[0])
    same64("stats", o["stats"], [r["costs"].min(), e.sum(), (e * e).sum(), (e * r["costs"].astype(f64)).sum()])
    same64("states", o["states"], oracle_problem(family, 1, pb.T).rollout_single(pb.x0, o["action"].astype(f32)))
    same64("warm start", o["carry"]["mean"], o["action"].astype(f32))
    same64("next state", o["carry"]["x"], o["states"][1])
    same64("sigma table stays", o["sigma"], np.tile(pb.sigmas, (pb.T, 1)))


def test_anchor_models_are_their_references():
    """The three table-driven families: costs of one plain tick, float64 and float32, are the family's reference on the same U"""
    for family in ("nav_soft", "racing_discs", "mlp42"):
        pb = one_feature(None, family)
        m = pb.model
        for dtype in (f64, f32):
            _, _, o = first_tick(pb, dtype)
            U = o["U"]
            if family == "nav_soft":
                want = SD.rollout_nav2d(m.P, m.grid, m.table, pb.x0, U, m.ab[0], m.ab[1], dtype)["costs"]
            elif family == "racing_discs":
                want = RD.rollout(m.P, m.grids, m.ref, m.table, pb.x0, U, dtype)["costs"]
            else:
                cs = m.cs
                want = ML.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], pb.x0, U, dtype)[0]
            same64(f"{family} {dtype.__name__}", o["costs"], want)


def test_anchor_action_cost():
    pb = one_feature("AC", "pendulum")
    plain = pb.without("AC")
    carry, eps, o = first_tick(pb)
    c0 = sr.tick(plain, carry, eps)["costs"]
    g = acref.g32(carry["mean"], pb.sigmas)
    kappa = acref.kappa32(sr.AC_WEIGHT, pb.lams[0])
    same64("float64", o["costs"], c0 + float(kappa) * acref.A64(g, o["U"].astype(f32))[0])
    o32 = sr.tick(pb, carry, eps, f32)
    c32 = sr.tick(plain, carry, eps, f32)["costs"]
    same64("float32", o32["costs"], acref.total32(c32, kappa, acref.A32(g, o32["U"])))
    assert np.any(o["costs"] != c0)


def test_anchor_correlated_draw():
    pb = one_feature("CN", "nav_soft")
    carry = pb.carry0()
    xi = NP(1, 0, pb.N, pb.T * pb.dc).reshape(pb.N, pb.T, pb.dc).astype(f32)
    got = sr.eps_for(pb, carry, 1, normals=NP)
    assert got.dtype == f32 and np.array_equal(got, colored(xi, sr.BETA, pb.sigmas))
    assert not np.array_equal(got, (xi * pb.sigmas).astype(f32))
    # ... and the float64 form of the same recurrence stays within the fp32 statement's rounding of it
    z64 = sr.draw(1, 0, pb.N, pb.T, pb.dc, pb.beta, carry["sigma"], f64, normals=NP)
    assert np.abs(z64 - got).max() <= 8 * 2.0 ** -24 * np.abs(z64).max()


def test_anchor_covariance():
    pb = one_feature("CV", "cartpole")
    carry, eps, o = first_tick(pb)
    cv = pb.cov
    want, var = restate(o["U"], o["costs32"], pb.lams[0], carry["sigma"], rate=cv["rate"], floor=cv["floor"], smin=cv["smin"], smax=cv["smax"])
    same64("float64 table", o["sigma"], want)
    assert np.any(o["sigma"] != carry["sigma"])
    o32 = sr.tick(pb, carry, eps, f32)
    full = lambda v: np.broadcast_to(f32(v), (pb.T, pb.dc)).ravel()  # noqa: E731
    s32 = numpy_step((carry["sigma"] ** 2).ravel(), o32["var"].ravel(), full(cv["rate"]), full(cv["floor"]), full(cv["smin"]), full(cv["smax"]))
    assert np.array_equal(o32["sigma"].ravel(), s32)
    same64("the next draw uses it", o["carry"]["sigma"], want.astype(f32))


def test_anchor_particles():
    for family in ("pendulum", "nav_soft"):
        pb = one_feature("PR", family)
        carry, eps, o = first_tick(pb)
        parts = pb.particles(carry["x"])
        assert parts.shape == (3, pb.ds) and np.array_equal(parts[0], carry["x"])
        assert np.any(o["matrix"].max(0) > o["matrix"][0]), "the nominal state is not the worst particle of every sample"
        plain = pb.without("PR")
        for m, x in enumerate(parts):
            same64(f"row {m}", o["matrix"][m], sr.tick(plain, dict(carry, x=x), eps)["costs"])
        same64("fold64", o["costs"], pc.fold64(o["matrix"], *pb.risk))
        o32 = sr.tick(pb, carry, eps, f32)
        assert np.array_equal(o32["costs"], _host.fold_particle_costs(o32["matrix"], *pb.risk))
        same64("the batch-1 rollout starts at the nominal state", o["states"][0], carry["x"])


def test_anchor_exploration():
    pb = one_feature("EX", "pendulum")
    carry, eps, o = first_tick(pb, f32)
    r = oracle_problem("pendulum", pb.N, pb.T, exploration=sr.EXPLORATION).rollout_cost(pb.x0, carry["mean"], eps, want_U=True)
    assert pb.inherit == int(pb.N * (1 - sr.EXPLORATION)) < pb.N
    assert np.array_equal(o["U"], r["U"]) and np.array_equal(o["costs"], r["costs"])


def test_anchor_filter():
    pb = one_feature("SG", "cartpole")
    carry = pb.carry0()
    carry["hist"] = (0.1 * np.random.default_rng(3).standard_normal((pb.T - 1, pb.dc))).astype(f32)
    eps = sr.eps_for(pb, carry, 1, normals=NP)
    o = sr.tick(pb, carry, eps)
    raw = softmax_action(o["costs32"], pb.lams[0], o["U"])
    want = _host.sg_filter_sequence(carry["hist"], raw, pb.sg)
    assert np.array_equal(o["action"], want) and not np.array_equal(want, raw.astype(f32))
    assert np.array_equal(o["hist"], np.concatenate([carry["hist"][1:], want[:1]]))
    same64("pre-filter mean", o["mean_w"], raw)


@pytest.mark.parametrize("rule", sr.RULES)
def test_anchor_temperature(rule):
    pair = next(p for p in sr.PAIRS if sr.rotation()[p][1] == rule)
    model, x0 = sr.host_model(sr.rotation()[pair][0])
    pb = sr.Problem(pair, model, x0, {"TL"})
    outs = sr.closed_loop(pb, normals=NP)
    p, lo, hi = pb.rule_args()
    prev, state = 0.0, np.array([float(f32(np.log(pb.lams[0]))), 0.0, 0.0, 0.0])
    for o in outs:
        c = o["costs32"]
        if rule == "ESSPS":
            want = emul.essps(c, p, lo, hi, lam_prev=prev, grid_argument=True)
            assert lo < want < hi and abs(weights64(c, want)[1] - p) <= 1e-4 * p
        elif rule == "LBPS_BRENT":
            want = emul.lbps(c, p, lo, hi)[0]
        elif rule == "LBPS_GRID":
            want = emul.lbps_grid(c, p, lo, hi)
        else:
            want = float(f32(pb.lams[0])) if not prev else nxt
            state, nxt = emul.mpo_step_stats(state, sr.MPO_EPS, sr.MPO_LR, sr.stats5(c, sr.softplus32(state[0])))
        assert o["lambda"] == want, (rule, o["lambda"], want)
        prev = want
    assert len({o["lambda"] for o in outs}) == len(outs)


def test_anchor_sharding():
    """Two windows of the global samples: their U and costs are the halves of the unsharded tick's, and the combined tail is
    the unsharded tail, bit for bit (the same float64 sums over the same values)."""
    pb = one_feature("SH", "pendulum")
    carry = pb.carry0()
    whole = sr.tick(pb, carry, sr.eps_for(pb, carry, 1, normals=NP))
    both = sr.tick_sharded(pb, carry, 1, normals=NP)
    h = pb.N // 2
    for r, part in enumerate(both["shards"]):
        same64(f"window {r}: U", part["U"], whole["U"][r * h:(r + 1) * h])
        same64(f"window {r}: costs", part["costs"], whole["costs"][r * h:(r + 1) * h])
    for key in ("action", "states", "stats", "sigma"):
        same64(key, both[key], whole[key])
    lost = sr.tick_sharded(pb, carry, 1, normals=NP, drop_offset=True)
    assert not np.array_equal(lost["shards"][1]["costs"], whole["costs"][h:])


# ---------------------------------------------------------------------------------------------- (b) sensitivity
def variants(pair, feature):
    """The wrong restatements that `feature` of `pair` must be told apart from"""
    other = pair[1] if pair[0] == feature else pair[0]
    out = ["drop"]
    if feature == "AC" and other == "CV":
        out.append("g_base_sigma")
    if {feature, other} == {"CN", "CV"}:
        out.append("scale_then_filter")
    if feature == "CV" and other == "SG":
        out.append("var_on_filtered")
    if feature == "CV" and other == "EX":
        out.append("explore_inherits_in_var")
    if {feature, other} == {"EX", "SH"}:
        out.append("local_inherit")
    if {feature, other} == {"PR", "TL"}:
        out.append("search_on_particle0")
    if feature == "PR" and sr.host_problem(pair).risk[0] == "worst":
        out.append("worst_as_mean")
    return out


SENSITIVITY = [(p, f, v) for p in sr.PAIRS for f in p for v in variants(p, f)]
_right = {}


def right_loop(pair):
    if pair not in _right:
        pb = sr.host_problem(pair)
        _right[pair] = (pb, sr.closed_loop(pb, normals=NP, sharded="SH" in pair))
    return _right[pair]


def test_every_wrong_variant_is_used():
    assert {v for _, _, v in SENSITIVITY} == set(sr.WRONG) | {"drop"}
    assert {(p, f) for p, f, _ in SENSITIVITY} == {(p, f) for p in sr.PAIRS for f in p}


@pytest.mark.parametrize("pair,feature,variant", SENSITIVITY, ids=[f"{sr.pair_id(p)}-{f}-{v}" for p, f, v in SENSITIVITY])
def test_a_wrong_restatement_moves_a_compared_quantity_ten_limits(pair, feature, variant):
    pb, right = right_loop(pair)
    sharded = "SH" in pair
    if variant == "drop" and feature == "SH":
        wrong = sr.closed_loop(pb, normals=NP, sharded=True, drop_offset=True)
    elif variant == "drop":
        wrong = sr.closed_loop(pb.without(feature), normals=NP, sharded=sharded)
    else:
        wrong = sr.closed_loop(pb, wrong=(variant,), normals=NP, sharded=sharded)
    worst = {}
    for a, b in zip(wrong, right):
        d = sr.distances(a, b, pb)
        if feature in ("CN", "CV", "EX", "SH") and a["U"].shape == b["U"].shape:  # the pairs that are about the draw: U is compared too
            d["noise"] = float(np.max(np.abs(a["U"].astype(f64) - b["U"]))) / (10 * 2.0 ** -24 * float(np.abs(b["U"]).max()))
        for k, v in d.items():
            worst[k] = max(worst.get(k, 0.0), v)
    top = max(worst, key=worst.get)
    print(f"[pairs] {sr.pair_id(pair)} {feature} {variant}: moves {top} by {worst[top]:.3g} limits; " +
          ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert worst[top] >= 10.0, (pair, feature, variant, worst)


# ---------------------------------------------------------------------------------------------- (c) the cap, and well-posed cases
@pytest.mark.parametrize("pair", sr.PAIRS, ids=IDS)
def test_cases_are_well_posed(pair):
    """Per tick: boundary samples within the cap from the float64 and the float32 restatement alone, the ESS inside the window
    that makes the weighted sums sums, every output finite; printed: the distance of the float32 from the float64
    restatement on the case's inputs (what profiles/feature_pairs.md quotes where a limit is rounding-bound)."""
    pb, loop64 = right_loop(pair)
    loop32 = sr.closed_loop(pb, f32, normals=NP, sharded="SH" in pair)
    cap = sr.boundary_cap(pb.N)
    lo, hi = sr.ess_window(pb.N)
    carry = pb.carry0()
    for t, (o64, o32) in enumerate(zip(loop64, loop32)):
        # (the fp32 loop carries no boundary notion of its own: its inputs are judged by the float64 rollout)
        at32 = sr.tick(pb, carry, sr.eps_for(pb, carry, t + 1, normals=NP)) if "SH" not in pair else o64
        left64, left32 = int(o64["boundary"].sum()), int(at32["boundary"].sum())
        d = sr.distances(o32, o64, pb)
        print(f"[pairs] {sr.pair_id(pair)} tick {t}: ESS {o64['ess']:.1f} of {pb.N}, lambda {o64['lambda']:.5g}, boundary {left64} / {left32} "
              f"(cap {cap}); float32 against float64, in limits: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(d.items())))
        assert left64 <= cap and left32 <= cap, (pair, t, left64, left32)
        assert lo <= o64["ess"] <= hi, (pair, t, o64["ess"])
        for key in ("costs", "action", "states", "sigma", "stats", "top_states", "top_weights"):
            assert np.all(np.isfinite(np.asarray(o64[key], f64))), (pair, t, key)
        carry = o32["carry"]
    if "AC" in pair:
        assert all(o["kappa"] > 0 for o in loop64[1:]) and np.any(loop64[-1]["g"] != 0)
    if "CV" in pair:
        assert not np.array_equal(loop64[-1]["sigma"], loop64[0]["sigma"])
        s = loop64[1]["carry"]["sigma"]
        assert np.ptp(s[:, 0]) > 0.02 * s[:, 0].mean(), "a non-constant table: filter-then-scale differs from scale-then-filter"
