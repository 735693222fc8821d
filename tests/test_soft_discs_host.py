"""The two soft disc models (MPPI_MODEL_NAV2D_DISCS_SOFT / MPPI_MODEL_RACING_DISCS_SOFT) without a GPU: the functor text of
csrc/mppi_models.inc and csrc/mppi_discs.hpp compiled with g++ (tests/host_emul/soft_discs_emul.cpp) against the numpy
restatement of tests/soft_discs_ref.py, the claims the GPU test relies on, and the soft envs on CPU tensors.

  the tables (discs_ref / racing_discs_ref, unchanged) under the soft rule, in float64 on 512 samples per case: the boundary
    rule leaves out at most cap samples, the mixed cases exercise the ramp (>= 5 % of the samples visit a skirt with 0 < ramp at
    T >= 7), and the fp32 restatement stays within PARITY / 4 of float64 on the same states (with skirt = 1 without any `near`
    exclusion).  Measured: at most 3.1e-7 (nav2d) and 2.2e-7 (racing) of the cost scale over the four settings.
  math level 0: states and costs equal the fp32 restatement BIT FOR BIT on every case and horizon.
  math level 1: costs within PARITY of the cost scale of float64 (evaluated on the functor's own states) for every sample the
    boundary rule keeps; on its own states the functor equals the spelled-out FMA restatement bit for bit.
  skirt = 0 equals the hard functor bit for bit at both levels; an empty table or a table nobody reaches equals plain nav2d /
    racing bit for bit.
  The same program with its own main, built with -fsanitize=address,undefined, walks the cases.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import discs_ref as D
import racing_discs_ref as RD
import soft_discs_ref as R
from helpers import nav2d_env_fixture, orc, racing_env_fixture

f32, f64 = np.float32, np.float64
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
SRC = os.path.join(HERE, "soft_discs_emul.cpp")
N_HOST = 100
MODELS = ("nav2d", "racing")
_world = {}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def world(model):
    if model not in _world:
        if model == "nav2d":
            e = nav2d_env_fixture()
            grid = (np.ascontiguousarray(e["map"], np.uint8), float(e["cell"]), float(e["origin"][0]), float(e["origin"][1]))
            _world[model] = dict(P=f32(orc.nav2d_params()), grids=(grid,))
        else:
            e = racing_env_fixture()
            geom = (float(e["cell"]), float(e["origin"][0]), float(e["origin"][1]))
            _world[model] = dict(P=f32(orc.racing_params()), start=f32(e["start_state"]), path=f32(e["center_path"]),
                                 x_hi=float(e["x_lim"][1]),
                                 grids=tuple((np.ascontiguousarray(e[k], np.uint8),) + geom for k in ("obst", "lane")))
    return _world[model]


def cases(model):
    return list((D if model == "nav2d" else RD).CASES)


def mixed(model):
    return (D if model == "nav2d" else RD).MIXED


def case(model, name, T):
    """-> (table, x0, ref or None)"""
    if model == "nav2d":
        table, x0 = D.case(name, T)
        return table, x0, None
    w = world(model)
    table, x0 = RD.case(name, T, w["start"], w["x_hi"])
    return table, x0, RD.window(w["path"], w["start"], T)


def actions(model, seed, N, T):
    return (D if model == "nav2d" else RD).actions(seed, N, T)


def restate(model, table, x0, ref, U, ab, **kw):
    w = world(model)
    if model == "nav2d":
        return R.rollout_nav2d(w["P"], w["grids"][0], table, x0, U, ab[0], ab[1], **kw)
    return R.rollout_racing(w["P"], w["grids"], ref, table, x0, U, ab[0], ab[1], **kw)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("soft_discs_emul") / "libsoft_discs_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, SRC])
    lib = C.CDLL(so)
    i, f, vp = C.c_int, C.c_float, C.c_void_p
    lib.soft_discs_emul_nav2d.argtypes = [i, i, f, f, vp, vp, i, i, f, f, f, vp, i, i, vp, vp, i, i, vp, vp]
    lib.soft_discs_emul_racing.argtypes = [i, i, f, f, vp, vp, vp, i, i, f, f, f, vp, vp, i, i, vp, vp, i, i, vp, vp]

    def rollout(model, table, x0, ref, U, ab=(0.0, 0.0), fast=0, kind=0):
        """kind: 0 the soft functor with the coefficients ab, 1 the hard disc functor, 2 plain nav2d / racing"""
        w = world(model)
        N, T, _ = U.shape
        U = np.ascontiguousarray(U, f32)
        x = np.ascontiguousarray(x0, f32)
        costs, S = np.empty(N, f32), np.empty((N, T + 1, len(x)), f32)
        g = w["grids"]
        if model == "nav2d":
            d8 = np.ascontiguousarray(D.padded(table))
            rc = lib.soft_discs_emul_nav2d(int(fast), int(kind), float(ab[0]), float(ab[1]), _p(w["P"]), _p(g[0][0]), g[0][0].shape[0],
                                           g[0][0].shape[1], g[0][1], g[0][2], g[0][3], _p(d8), d8.shape[0], table.shape[1], _p(x), _p(U),
                                           N, T, _p(costs), _p(S))
        else:
            ref8 = np.ascontiguousarray(RD.ref_rows(ref), f32)
            rows = min(ref8.shape[0], table.shape[0])
            d8 = np.ascontiguousarray(RD.padded(table)[:rows])
            rc = lib.soft_discs_emul_racing(int(fast), int(kind), float(ab[0]), float(ab[1]), _p(w["P"]), _p(g[0][0]), _p(g[1][0]),
                                            g[0][0].shape[0], g[0][0].shape[1], g[0][1], g[0][2], g[0][3], _p(ref8), _p(d8), rows,
                                            table.shape[1], _p(x), _p(U), N, T, _p(costs), _p(S))
        assert rc == 0
        return costs, S

    out = (C.c_int * 10)()
    lib.soft_discs_emul_facts(out)
    rollout.facts = list(out)
    return rollout


# ------------------------------------------------------------------------------ the binding's facts
def test_ids_dims_slots(emul):
    from mppi_playground_amd import _capi

    nav_id, rac_id, krow_nav, krow_rac, slot_nav, slot_rac, count_slot, seq_nav, seq_rac, predicates = emul.facts
    assert (nav_id, rac_id) == (11, 12) == (_capi.MODEL_IDS["nav2d_discs_soft"], _capi.MODEL_IDS["racing_discs_soft"])
    assert _capi.MODEL_DIMS["nav2d_discs_soft"] == (3, 2) and _capi.MODEL_DIMS["racing_discs_soft"] == (4, 2)
    assert _capi.MODEL_IDS["nav2d_discs"] == 9 and _capi.MODEL_IDS["racing_discs"] == 10 and _capi.ABI_VERSION == 16
    assert {"mppi_set_disc_softness", "mppi_get_disc_softness"} <= set(_capi.SYMBOLS)
    assert (krow_nav, krow_rac) == (D.KROW, RD.KROW) == (32, 40)     # the hard models' rows: no new layout
    assert slot_nav == 12 and slot_nav + 1 < 32                      # behind nav2d's 12 parameters
    assert slot_rac == count_slot + 1 and count_slot == 17 and slot_rac + 1 < 32  # behind racing's disc count
    assert (seq_nav, seq_rac) == (0, 1)                              # nav2d's double accumulator, racing's sequential sum
    assert predicates == 1


def test_soft_coefficients_match_the_double_formula():
    from envs.discs import check_softness, soft_coefficients

    for reach, skirt in R.SETTINGS + (R.HARD, (1.0000001, 1.0), (1e6, 0.3)):
        k, phi = float(f32(reach)) ** 2, float(f32(skirt))
        a, b = soft_coefficients(reach, skirt)
        assert (f32(a), f32(b)) == (f32(phi * k / (k - 1.0)), f32(phi / (k - 1.0))) == R.coefficients(reach, skirt)
        assert float(f32(a)) == a and float(f32(b)) == b  # fp32 values, handed on as Python floats
    assert soft_coefficients(2.0, 1.0) == (float(f32(4.0 / 3.0)), float(f32(1.0 / 3.0)))
    assert soft_coefficients(2.0, 0.0) == (0.0, 0.0)
    for bad in ((1.0, 1.0), (0.5, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (2.0, -0.1), (2.0, 1.1), (2.0, float("nan"))):
        with pytest.raises(ValueError):
            check_softness(*bad)


def test_the_rule_itself():
    """the penalty as a function of the distance: w inside, skirt * w just outside, linear in d2, 0 from reach * r on"""
    r, w = 0.5, 8.0
    row = f32([[0.0, 0.0, r * r, w]])
    for reach, skirt in R.SETTINGS:
        a, b = R.coefficients(reach, skirt)
        d = f64([0.0, 0.3, r * (1 + 1e-6), r * np.sqrt((1 + reach * reach) / 2), reach * r * (1 - 1e-6), reach * r * 1.01, 50.0])
        pen, hit, skirted = R.soft_penalty(row, 1, d, np.zeros_like(d), a, b, f64)
        want = [w, w, skirt * w, 0.5 * skirt * w, 0.0, 0.0, 0.0]
        assert np.allclose(pen, want, atol=1e-4 * w), (reach, skirt, pen)
        assert list(hit[:, 0]) == [True, True] + [False] * 5 and list(skirted[:, 0]) == [False, False, True, True, True, False, False]


# ------------------------------------------------------------------------------ the tables' claims under the soft rule
@pytest.mark.parametrize("model", MODELS)
def test_table_claims(model):
    worst = {s: 0.0 for s in R.SETTINGS}
    for T in R.ALL_T:
        U = actions(model, 100 + T, 512, T)
        for name in cases(model):
            table, x0, ref = case(model, name, T)
            for setting in R.SETTINGS:
                ab = R.coefficients(*setting)
                r64 = restate(model, table, x0, ref, U, ab, dtype=f64)
                left = int(r64["near"].sum())
                assert left <= R.cap(len(U)), f"{model} {name} T{T}: the boundary rule would leave out {left} samples"
                share = float(r64["skirted"].any(axis=(1, 2)).mean()) if table.shape[1] else 0.0
                if name in mixed(model) and T >= 7:
                    assert share >= 0.05, f"{model} {name} T{T} {setting}: only {share:.3f} of the samples visit a skirt"
                if T >= 7:  # the fp32 restatement against float64 on the same states (soft_discs_ref: why the same states)
                    r32 = restate(model, table, x0, ref, U, ab)
                    s64 = restate(model, table, x0, ref, U, ab, dtype=f64, states=r32["S"])
                    keep = ~s64["edge"] if setting[1] == 1.0 else ~(s64["near"] | s64["edge"])  # skirt = 1: continuous at the rim
                    err = float(np.max(np.abs(r32["costs"].astype(f64) - s64["costs"])[keep]) / s64["scale"])
                    worst[setting] = max(worst[setting], err)
                    assert err <= R.PARITY / 4, f"{model} {name} T{T} {setting}: fp32 restatement {err:.3g} of the scale from float64"
    print(f"[soft discs] {model}: fp32 restatement against float64, worst share of the scale per setting: "
          + ", ".join(f"{s}: {e:.3g}" for s, e in worst.items()))


# ------------------------------------------------------------------------------ level 0: bit for bit
@pytest.mark.parametrize("model", MODELS)
def test_level0_equals_the_fp32_restatement(emul, model):
    for name in cases(model):
        for T in R.ALL_T:
            table, x0, ref = case(model, name, T)
            U = actions(model, 7 + T, N_HOST, T)
            for setting in ((2.0, 0.25), (3.0, 0.5)) if T != 8 else R.SETTINGS:
                ab = R.coefficients(*setting)
                c, S = emul(model, table, x0, ref, U, ab)
                r32 = restate(model, table, x0, ref, U, ab)
                assert np.array_equal(bits(S), bits(r32["S"])), f"{model} {name} T={T} {setting}: states"
                assert np.array_equal(bits(c), bits(r32["costs"])), f"{model} {name} T={T} {setting}: costs"
                assert np.all(np.isfinite(c))


# ------------------------------------------------------------------------------ level 1: the parity rule
@pytest.mark.parametrize("model", MODELS)
def test_level1_within_the_parity_rule(emul, model):
    for name in cases(model):
        for T in R.ALL_T:
            table, x0, ref = case(model, name, T)
            U = actions(model, 11 + T, N_HOST, T)
            for setting in ((2.0, 1.0), (2.0, 0.25)) if T != 8 else R.SETTINGS:
                ab = R.coefficients(*setting)
                c, S = emul(model, table, x0, ref, U, ab, fast=1)
                r64 = restate(model, table, x0, ref, U, ab, dtype=f64, states=S)  # (float64 on the functor's own states)
                keep = ~(r64["near"] | r64["edge"])
                assert int(r64["near"].sum()) <= R.cap(N_HOST)
                err = np.abs(c.astype(f64) - r64["costs"])[keep]
                assert np.all(err <= R.PARITY * r64["scale"]), \
                    f"{model} {name} T={T} {setting}: {err.max():.3g} against {R.PARITY * r64['scale']:.3g}"
                own = restate(model, table, x0, ref, U, ab, states=S, fuse=True)  # the spelled-out FMAs on the functor's own states
                assert np.array_equal(bits(c), bits(own["costs"])), f"{model} {name} T={T} {setting}: level-1 costs on the functor's states"


# ------------------------------------------------------------------------------ skirt = 0, empty tables, tables nobody reaches
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_skirt_zero_equals_the_hard_functor(emul, model, fast):
    ab = R.coefficients(*R.HARD)
    assert ab == (0.0, 0.0)
    some_hit = False
    for name in cases(model):
        for T in R.ALL_T:
            table, x0, ref = case(model, name, T)
            U = actions(model, 3 + T, N_HOST, T)
            c, S = emul(model, table, x0, ref, U, ab, fast=fast)
            ch, Sh = emul(model, table, x0, ref, U, fast=fast, kind=1)
            assert np.array_equal(bits(c), bits(ch)) and np.array_equal(bits(S), bits(Sh)), f"{model} {name} T={T} fast={fast}"
            cp, _ = emul(model, table, x0, ref, U, fast=fast, kind=2)
            some_hit |= not np.array_equal(bits(c), bits(cp))
    assert some_hit  # (the discs were charged: the equality above is not plain nav2d / racing three times)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_no_discs_and_all_miss_equal_the_plain_functor(emul, model, fast):
    far = (D if model == "nav2d" else RD).FAR
    for T in R.ALL_T:
        _, x0, ref = case(model, "n0", T)
        U = actions(model, 3 + T, N_HOST, T)
        cp, Sp = emul(model, np.zeros((T, 0, 4), f32), x0, ref, U, fast=fast, kind=2)
        for setting in R.SETTINGS:  # (the widest skirt ends 3 x 0.2 m from a centre 40 m and more away)
            for table in (np.zeros((T, 0, 4), f32), np.broadcast_to(far, (T, 8, 4)).copy()):
                c, S = emul(model, table, x0, ref, U, R.coefficients(*setting), fast=fast)
                assert np.array_equal(bits(c), bits(cp)) and np.array_equal(bits(S), bits(Sp)), f"{model} T={T} n={table.shape[1]} {setting}"


# ------------------------------------------------------------------------------ the restatement can fail
@pytest.mark.parametrize("model", MODELS)
def test_the_restatement_can_fail(model):
    """The cases tell a wrong reading of the rule apart: a ramp in d instead of d2, a skirt that also scales the inside,
    a and b swapped."""
    T = 8
    U = actions(model, 5, 256, T)
    table, x0, ref = case(model, "n3", T)
    for reach, skirt in ((2.0, 0.25), (3.0, 0.5)):
        ab = R.coefficients(reach, skirt)
        right = restate(model, table, x0, ref, U, ab)["costs"]
        for wrong in R.WRONG:
            got = restate(model, table, x0, ref, U, ab, wrong=wrong, reach=reach, skirt=skirt)["costs"]
            assert not np.array_equal(right, got), f"{model} {(reach, skirt)}: {wrong} goes unnoticed"
            assert np.mean(right != got) >= 0.05, f"{model} {(reach, skirt)}: {wrong} shows in {np.mean(right != got):.3f} of the samples only"


# ------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_passes_the_sanitizers(emul, tmp_path):
    exe = str(tmp_path / "soft_discs_emul_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-DSOFT_DISCS_EMUL_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    want, blob = [], bytearray()
    ab = R.coefficients(2.0, 0.25)
    for model in MODELS:
        w = world(model)
        g = w["grids"]
        for name in cases(model):
            for T in (1, 3, 8):
                for fast in (0, 1):
                    table, x0, ref = case(model, name, T)
                    U = actions(model, 5, 64, T)
                    hd = np.array([model == "racing", fast, 0, 64, T, T, table.shape[1], g[0][0].shape[0], g[0][0].shape[1]], np.int32)
                    blob += hd.tobytes() + f32(ab).tobytes() + w["P"].tobytes() + f32(g[0][1:]).tobytes()  # exactly T rows
                    blob += b"".join(m[0].tobytes() for m in g)
                    if model == "racing":
                        blob += RD.ref_rows(ref)[:T].astype(f32).tobytes()
                    blob += D.padded(table)[:T].tobytes() + f32(x0).tobytes() + U.tobytes()
                    want.append(emul(model, table, x0, ref, U, ab, fast=fast)[0])
    (tmp_path / "cases.bin").write_bytes(bytes(blob))
    out = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "costs.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    assert f"{len(want)} cases" in out.stdout
    got = np.fromfile(str(tmp_path / "costs.bin"), f32)
    assert np.array_equal(bits(got), bits(np.concatenate(want)))


# ------------------------------------------------------------------------------ the environments, on CPU tensors
def test_nav2d_env_cost_equals_the_restatement():
    import torch

    from envs import SoftMovingObstacleNav2DEnv

    T = 8
    env = SoftMovingObstacleNav2DEnv(horizon=T, soft_reach=3.0, soft_skirt=0.5, device=torch.device("cpu"))
    assert (env.soft_reach, env.soft_skirt) == (3.0, 0.5)
    m = env._obstacle_map.grid_spec()
    grid = (np.ascontiguousarray(m.cells, np.uint8), float(m.cell_size), float(m.origin[0]), float(m.origin[1]))
    spec = type(env).cost_function.__mppi_native__.provider(env)
    assert spec["discs"]["soft"] == {"reach": 3.0, "skirt": 0.5} and spec["discs"]["table"] is env._disc_table and len(spec["params"]) == 12
    P = f32(spec["params"])
    table, _ = D.case("weights8", T)
    env._disc_table = torch.from_numpy(table.copy())
    rng = np.random.default_rng(1)
    s = np.concatenate([table[3, 0, :2] + rng.uniform(-0.4, 0.4, (300, 2)), rng.uniform(-3, 3, (300, 1))], 1).astype(f32)
    for setting in ((3.0, 0.5), (2.0, 1.0), (2.0, 0.0)):
        env.set_softness(*setting)
        a, b = R.coefficients(*setting)
        got = env.cost_function(torch.from_numpy(s), torch.zeros(300, 2), {"t": 3}).numpy()
        pen, hit, skirted = R.soft_penalty(table[3], 8, s[:, 0], s[:, 1], a, b)
        assert 0.05 < hit.any(1).mean() < 0.95 and (setting[1] == 0.0 or skirted.any(1).mean() > 0.05)
        assert np.array_equal(bits(got), bits((D.base_cost(P, grid, s) + pen).astype(f32))), setting
    hard = D.base_cost(P, grid, s) + D.penalty(table[3], 8, s[:, 0], s[:, 1])[0]
    assert np.array_equal(bits(got), bits(hard.astype(f32)))  # skirt = 0: the hard env's cost
    inside = torch.tensor([[[float(table[0, 0, 0]), float(table[0, 0, 1]), 0.0]]])
    skirt_only = torch.tensor([[[float(table[0, 0, 0]) + 0.3, float(table[0, 0, 1]), 0.0]]])  # r = 0.2: outside the disc
    assert float(env.collision_check(inside)) >= 1.0 and float(env.collision_check(skirt_only)) == 0.0  # the hard test
    with pytest.raises(ValueError):
        env.set_softness(1.0, 0.5)
    with pytest.raises(ValueError):
        env.set_softness(2.0, 1.5)
    with pytest.raises(ValueError):
        env.set_moving_obstacles(torch.zeros(2, 2), torch.zeros(2, 2), [0.3, 0.0])
    with pytest.raises(ValueError):
        SoftMovingObstacleNav2DEnv(horizon=T, soft_reach=float("inf"), device=torch.device("cpu"))
    env.set_moving_obstacles(torch.zeros(2, 2), torch.zeros(2, 2), [0.3, 0.2])
    assert env.predict_discs().shape == (T, 2, 4)


def test_racing_controller_cost_equals_the_restatement():
    import torch

    from envs.racing_opponents import SoftOpponentRacingEnv, soft_opponent_racing_controller

    T, t = 8, 3
    env = SoftOpponentRacingEnv(horizon=T, soft_reach=2.0, soft_skirt=0.25, device=torch.device("cpu"))
    ctrl = soft_opponent_racing_controller(env, device=torch.device("cpu"), horizon=T, num_samples=64, mppi_cls=lambda **kw: None)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    x0 = RD.start_pose(env.reset().numpy())
    ref = RD.window(env.racing_center_path_np, x0, T)
    ctrl.set_reference(ref)
    table = RD.case("overlap2", T, x0)[0]
    env._opp_table = torch.from_numpy(table.copy())
    spec = type(ctrl).cost_function.__mppi_native__.provider(ctrl)
    assert spec["discs"]["soft"] == {"reach": 2.0, "skirt": 0.25} and spec["discs"]["table"] is env._opp_table and len(spec["params"]) == 17
    grids = tuple((np.ascontiguousarray(g.cells, np.uint8), float(g.cell_size), float(g.origin[0]), float(g.origin[1]))
                  for g in spec["maps"])
    rng = np.random.default_rng(1)
    s = np.concatenate([table[t, 0, :2] + rng.uniform(-0.6, 0.6, (300, 2)), rng.uniform(-3, 3, (300, 1)), rng.uniform(0, 8, (300, 1))],
                       1).astype(f32)
    u, pu = RD.actions(2, 300, 1)[:, 0], RD.actions(3, 300, 1)[:, 0]
    got = ctrl.cost_function(torch.from_numpy(s), torch.from_numpy(u), {"t": t, "prev_action": torch.from_numpy(pu)}).numpy()
    pen, hit, skirted = R.soft_penalty(table[t], 2, s[:, 0], s[:, 1], *R.coefficients(2.0, 0.25))
    base = RD.base_cost(f32(spec["params"]), grids, RD.ref_rows(ref)[t], s, u, pu)
    assert 0.05 < hit.any(1).mean() < 0.95 and skirted.any(1).mean() > 0.05
    # (torch's sum(dim=1) of two squares and its sin / cos of the reference yaw are one rounding each like the restatement's)
    assert np.allclose(got, (base + pen).astype(f32), rtol=1e-6, atol=0.0)
    assert np.allclose(got - pen, base, rtol=1e-6)
    with pytest.raises(ValueError):
        env.set_softness(0.5, 0.5)
    with pytest.raises(ValueError):
        env.set_opponents([10], [1.0], 0.0)
    inside = torch.cat([env._opp_table[0, 1, :2], torch.zeros(2)]).view(1, 1, 4)
    assert float(env.opponent_hits(inside)) == 2.0  # (two cars on one spot) the hard test


def test_tags_and_untagged_lambdas():
    import torch

    from envs import MovingObstacleNav2DEnv, SoftMovingObstacleNav2DEnv
    from envs.navigation_2d import Navigation2DEnv
    from envs.racing_controller import racing_controller
    from envs.racing_env import RacingEnv
    from envs.racing_opponents import (OpponentRacingEnv, SoftOpponentRacingEnv, opponent_racing_controller,
                                       soft_opponent_racing_controller)
    from pi_mpc.native import resolve

    cpu = torch.device("cpu")
    env = SoftMovingObstacleNav2DEnv(horizon=4, device=cpu)
    assert (env.soft_reach, env.soft_skirt) == (2.0, 1.0) and isinstance(env, MovingObstacleNav2DEnv)
    (dt, do), (ct, co) = resolve(env.dynamics), resolve(env.cost_function)
    assert (dt.model, dt.role, ct.model, ct.role) == ("nav2d_discs_soft", "dynamics", "nav2d_discs_soft", "cost") and do is env and co is env
    assert resolve(lambda s, a: env.dynamics(s, a)) is None
    renv = SoftOpponentRacingEnv(horizon=4, device=cpu)
    ctrl = soft_opponent_racing_controller(renv, device=cpu, horizon=4, num_samples=64, mppi_cls=lambda **kw: None)
    assert isinstance(renv, OpponentRacingEnv) and isinstance(ctrl, opponent_racing_controller)
    (dt, do), (ct, co) = resolve(renv.dynamics), resolve(ctrl.cost_function)
    assert (dt.model, dt.role, ct.model, ct.role) == ("racing_discs_soft", "dynamics", "racing_discs_soft", "cost") and do is renv and co is ctrl
    assert resolve(lambda s, a, i: ctrl.cost_function(s, a, i)) is None
    # the parents' tags are what they were
    assert MovingObstacleNav2DEnv.dynamics.__mppi_native__.model == MovingObstacleNav2DEnv.cost_function.__mppi_native__.model == "nav2d_discs"
    assert OpponentRacingEnv.dynamics.__mppi_native__.model == opponent_racing_controller.cost_function.__mppi_native__.model == "racing_discs"
    assert Navigation2DEnv.cost_function.__mppi_native__.model == "nav2d" and RacingEnv.dynamics.__mppi_native__.model == "racing"
    assert racing_controller.cost_function.__mppi_native__.model == "racing"
