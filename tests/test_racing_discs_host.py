"""Racing among moving discs (MPPI_MODEL_RACING_DISCS) without a GPU: the functor text of csrc/mppi_models.inc and
csrc/mppi_discs.hpp compiled with g++ (tests/host_emul/racing_discs_emul.cpp) against the numpy restatement of
tests/racing_discs_ref.py, the claims of the case table the GPU test shares, the layout of the handle's step table, and
envs.racing_opponents on CPU tensors.

  math level 0: states and costs equal the fp32 restatement BIT FOR BIT on every case and horizon; n = 0 and all-miss tables
    equal the plain racing functor bit for bit (at level 1 too).
  math level 1: costs within 2e-6 of the cost scale of the float64 restatement for every sample the boundary rule keeps.
  The same program with its own main, built with -fsanitize=address,undefined, walks the table's cases.
The maps, the parameters, the centre line and the start pose are racing's golden fixture (tests/golden/racing_env.npz).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import racing_discs_ref as R
from helpers import orc, racing_env_fixture

f32, f64 = np.float32, np.float64
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
SRC = os.path.join(HERE, "racing_discs_emul.cpp")
N_HOST = 100
_world = {}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def world():
    if not _world:
        e = racing_env_fixture()
        geom = (float(e["cell"]), float(e["origin"][0]), float(e["origin"][1]))
        _world.update(P=f32(orc.racing_params()), start=f32(e["start_state"]), path=f32(e["center_path"]), x_hi=float(e["x_lim"][1]),
                      grids=tuple((np.ascontiguousarray(e[k], np.uint8),) + geom for k in ("obst", "lane")))
    return _world


def case(name, T):
    """-> (table, x0, ref [T + 1, 4]): the window of the example's tick from the start pose"""
    w = world()
    table, x0 = R.case(name, T, w["start"], w["x_hi"])
    return table, x0, R.window(w["path"], w["start"], T)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("racing_discs_emul") / "libracing_discs_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.racing_discs_emul_rollout.argtypes = ([C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                               C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_int, C.c_void_p, C.c_void_p])
    w = world()
    g0, g1 = w["grids"]

    def rollout(table, x0, ref, U, fast=0, plain=0):
        N, T, _ = U.shape
        U = np.ascontiguousarray(U, f32)
        ref8 = np.ascontiguousarray(R.ref_rows(ref), f32)
        rows = min(ref8.shape[0], table.shape[0])
        d8 = np.ascontiguousarray(R.padded(table)[:rows])
        costs, S = np.empty(N, f32), np.empty((N, T + 1, 4), f32)
        x = np.ascontiguousarray(x0, f32)
        rc = lib.racing_discs_emul_rollout(int(fast), int(plain), _p(w["P"]), _p(g0[0]), _p(g1[0]), g0[0].shape[0], g0[0].shape[1],
                                           g0[1], g0[2], g0[3], _p(ref8), _p(d8), rows, table.shape[1], _p(x), _p(U), N, T,
                                           _p(costs), _p(S))
        assert rc == 0
        return costs, S

    out = (C.c_int * 8)()
    lib.racing_discs_emul_layout(out)
    rollout.layout = list(out)
    return rollout


def ref32(table, x0, ref, U, **kw):
    w = world()
    return R.rollout(w["P"], w["grids"], ref, table, x0, U, **kw)


# ------------------------------------------------------------------------------ the table's claims
def test_table_claims():
    w = world()
    assert set(R.CASES) >= {"n0", "n1", "n3", "n8", "step0", "terminal", "overlap2", "x0out"}
    assert R.SAMPLES == (64, 100, 4160) and R.HORIZONS == (1, 2, 3, 7, 8, 25) and R.COUNTS == (0, 1, 3, 8)
    assert {case(n, 8)[0].shape[1] for n in ("n0", "n1", "n3", "n8")} == set(R.COUNTS)
    x_out = case("x0out", 8)[1]
    assert not (w["P"][7] <= x_out[0] <= w["P"][8]) and w["P"][7] <= case("n3", 8)[1][0] <= w["P"][8]
    for T in R.HORIZONS:
        for name in R.CASES:
            table, x0, ref = case(name, T)
            for N in R.SAMPLES:  # the float64 restatement alone, at every sample count of the table
                left = int(ref32(table, x0, ref, R.actions(100 + T + N, N, T), dtype=f64)["near"].sum())
                assert left <= R.cap(N), f"{name} T{T} N{N}: the boundary rule would leave out {left} samples (cap {R.cap(N)})"
            U = R.actions(100 + T, 512, T)
            r64 = ref32(table, x0, ref, U, dtype=f64)
            hit = r64["hit"]
            left = int(r64["near"].sum())
            share = float(hit.any(axis=(1, 2)).mean()) if hit.size else 0.0
            print(f"[racing discs] table {name} T{T}: hit share {share:.3f}, left out {left} of {len(U)} (cap {R.cap(len(U))})")
            assert left <= R.cap(len(U)), f"{name} T{T}: the boundary rule would leave out {left} samples"
            if name in R.MIXED and T >= 7:  # both answers for some car
                per_disc = hit.any(1).mean(0)[table[0, :, 0] != R.FAR[0]]
                assert np.any((per_disc >= 0.05) & (per_disc <= 0.95)), f"{name} T{T}: hit share per disc {per_disc}"
            if name == "pace" and T >= 7:   # ... and at EVERY step from the fifth on, the terminal one included
                per_step = hit[:, :min(T + 1, R.PACE_ROWS), 0].mean(0)  # (T < PACE_ROWS: index T is the terminal cost on row T-1)
                assert np.all((per_step[5:] > 0) & (per_step[5:] < 1)) and hit[:, :2].all(), per_step
            if name == "step0":  # the start lies in the disc: every sample, at the start pose, nowhere else
                assert hit[:, 0].all() and not hit[:, 1:T].any() and (T == 1 or not hit[:, T].any())
            if name == "terminal":  # samples that reach it with their LAST step: only a terminal cost that reads row T-1 sees them
                assert (hit[:, T, 0] & ~hit[:, T - 1, 0]).mean() >= 0.05 and not hit[:, :T - 1].any()
            if name == "overlap2" and T >= 7:
                assert np.all(hit.sum(2)[hit.any(2)] == 2)
            if name == "slot7":
                assert not hit[:, :, :7].any()


# ------------------------------------------------------------------------------ the step table's layout
def test_combined_row_layout(emul):
    krow, ref_row, off, discs_t3, sequential, stride_discs, stride_plain, slot = emul.layout
    assert (krow, ref_row, off) == (R.KROW, R.REF_ROW, R.REF_ROW) == (40, 8, 8) and stride_discs == 40 and stride_plain == 8
    assert discs_t3 == 3 * R.KROW + R.REF_ROW == R.disc_float(3, 0)
    assert sequential == 1                      # racing's sequential fp32 cost sum, not the double accumulator
    assert 17 <= slot < 32                      # the count waits behind racing's 17 parameters, inside P[]
    for t in (0, 1, 24):
        for j in range(R.MAX_DISCS):
            assert (4 * R.disc_float(t, j)) % 16 == 0  # one 16-byte read per disc from a 16-byte-aligned table
    table, x0, ref = case("n3", 7)
    tab = R.combined(ref, table)
    assert tab.shape == (7, 40)
    assert np.array_equal(bits(tab[:, :4]), bits(ref[:7])) and np.all(tab[:, 6:8] == 0.0)
    assert np.array_equal(bits(tab[:, 4]), bits(R.ref_rows(ref)[:7, 4])) and np.array_equal(bits(tab[:, 5]), bits(R.ref_rows(ref)[:7, 5]))
    d = tab[:, 8:].reshape(7, 8, 4)
    assert np.array_equal(bits(d[:, :3]), bits(table)) and np.all(d[:, 3:, 2] == -1.0) and np.all(d[:, 3:, 3] == 0.0)
    assert np.all(d[:, 3:, :2] == 0.0)
    flat = tab.ravel()
    assert flat[R.disc_float(5, 2, 3)] == table[5, 2, 3] and flat[R.disc_float(6, 7, 2)] == -1.0


# ------------------------------------------------------------------------------ level 0: bit for bit
@pytest.mark.parametrize("name", list(R.CASES))
def test_level0_equals_the_fp32_restatement(emul, name):
    for T in R.HORIZONS:
        table, x0, ref = case(name, T)
        U = R.actions(7 + T, N_HOST, T)
        c, S = emul(table, x0, ref, U)
        r32 = ref32(table, x0, ref, U)
        assert np.array_equal(bits(S), bits(r32["S"])), f"{name} T={T}: states"
        assert np.array_equal(bits(c), bits(r32["costs"])), f"{name} T={T}: costs"
        assert np.all(np.isfinite(c))
        own = ref32(table, x0, ref, U, states=S)
        assert np.array_equal(bits(c), bits(own["costs"])), f"{name} T={T}: costs on given states"
        if name == "n0" or not r32["hit"].any():  # nothing hit: the plain racing functor's cost, bit for bit
            cp, Sp = emul(table, x0, ref, U, plain=1)
            assert np.array_equal(bits(c), bits(cp)) and np.array_equal(bits(S), bits(Sp)), f"{name} T={T}: plain racing"


@pytest.mark.parametrize("fast", [0, 1])
def test_no_discs_and_all_miss_equal_plain_racing(emul, fast):
    for T in R.HORIZONS:
        _, x0, ref = case("n0", T)
        U = R.actions(3 + T, N_HOST, T)
        cp, Sp = emul(np.zeros((T, 0, 4), f32), x0, ref, U, fast=fast, plain=1)
        for table in (np.zeros((T, 0, 4), f32), np.broadcast_to(R.FAR, (T, 8, 4)).copy()):
            c, S = emul(table, x0, ref, U, fast=fast)
            assert np.array_equal(bits(c), bits(cp)) and np.array_equal(bits(S), bits(Sp)), f"T={T} n={table.shape[1]} fast={fast}"


def test_the_restatement_can_fail():
    """The cases tell a wrong reading of the tables apart: disc row t + 1, reference row t + 1, no terminal row, one disc of two."""
    T = 8
    U = R.actions(5, 256, T)

    def differs(name, wrong_table=lambda t: t, wrong_ref=lambda r: r):
        table, x0, ref = case(name, T)
        return not np.array_equal(ref32(table, x0, ref, U)["costs"], ref32(wrong_table(table), x0, wrong_ref(ref), U)["costs"])

    assert differs("n3", lambda t: np.concatenate([t[1:], t[-1:]]))
    assert differs("n0", wrong_ref=lambda r: np.concatenate([r[1:], r[-1:]]))
    assert differs("terminal", lambda t: np.broadcast_to(R.FAR, t.shape))
    assert differs("overlap2", lambda t: t[:, :1])


# ------------------------------------------------------------------------------ level 1: the parity rule
@pytest.mark.parametrize("name", list(R.CASES))
def test_level1_within_the_parity_rule(emul, name):
    for T in R.HORIZONS:
        table, x0, ref = case(name, T)
        U = R.actions(11 + T, N_HOST, T)
        c, S = emul(table, x0, ref, U, fast=1)
        r64 = ref32(table, x0, ref, U, dtype=f64)
        keep = ~(r64["near"] | r64["edge"])
        assert int(r64["near"].sum()) <= R.cap(N_HOST)
        err = np.abs(c.astype(f64) - r64["costs"])[keep]
        print(f"[racing discs] host {name} T{T} math 1: left out {int((~keep).sum())}, max err {err.max() / r64['scale']:.3g} of the scale")
        assert np.all(err <= R.PARITY * r64["scale"]), f"{name} T={T}: {err.max():.3g} against {R.PARITY * r64['scale']:.3g}"


# ------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_passes_the_sanitizers(emul, tmp_path):
    exe = str(tmp_path / "racing_discs_emul_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-DRACING_DISCS_EMUL_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    w = world()
    g0, g1 = w["grids"]
    want, blob = [], bytearray()
    for name in R.CASES:
        for T in (1, 3, 8):
            for fast in (0, 1):
                table, x0, ref = case(name, T)
                U = R.actions(5, 64, T)
                hd = np.array([fast, 0, 64, T, T, table.shape[1], g0[0].shape[0], g0[0].shape[1]], np.int32)  # exactly T rows
                blob += (hd.tobytes() + w["P"].tobytes() + f32(g0[1:]).tobytes() + g0[0].tobytes() + g1[0].tobytes()
                         + R.ref_rows(ref)[:T].astype(f32).tobytes() + R.padded(table)[:T].tobytes() + f32(x0).tobytes() + U.tobytes())
                want.append(emul(table, x0, ref, U, fast=fast)[0])
    (tmp_path / "cases.bin").write_bytes(bytes(blob))
    out = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "costs.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    assert f"{len(want)} cases" in out.stdout
    got = np.fromfile(str(tmp_path / "costs.bin"), f32)
    assert np.array_equal(bits(got), bits(np.concatenate(want)))


# ------------------------------------------------------------------------------ the environment and the controller, on CPU tensors
def _env(T=8):
    import torch

    from envs.racing_opponents import OpponentRacingEnv

    return OpponentRacingEnv(horizon=T, device=torch.device("cpu"))


def test_env_table_equals_a_plain_loop_over_the_cars():
    import torch

    T = 6
    env = _env(T)
    assert env.predict_opponents().shape == (T, 0, 4)
    index, speed, radius, offset = [120, 200, 3670], [3.0, 1.55, 2.0], [0.5, 0.6, 0.45], [0.0, 1.25, -0.75]
    env.set_opponents(index, speed, radius, lateral_offset=offset)
    path, normal = env.racing_center_path, env._center_normal
    ticks = 0
    while True:
        tab = env._opp_table
        assert tab.shape == (T, 3, 4)
        for j in range(3):
            s_j = index[j] * env.dl + ticks * speed[j] * env.delta_t if ticks == 0 else float(env._opp_s[j])
            for t in range(T):
                i = min(int(round((s_j + speed[j] * (t * env.delta_t)) / env.dl)), path.shape[0] - 1)  # round(): half to even
                want = path[i, :2] + torch.tensor(offset[j]) * normal[i]
                assert torch.equal(tab[t, j, :2], want), (ticks, j, t)
                assert float(tab[t, j, 2]) == float(torch.tensor(radius[j]) * torch.tensor(radius[j]))
                assert float(tab[t, j, 3]) == env.opponent_weight
        if ticks == 2:
            break
        v0, ptr = env._opp_version, tab.data_ptr()
        env.step(torch.tensor([0.5, 0.0]))
        ticks += 1
        assert env._opp_version > v0 and env._opp_table.data_ptr() == ptr  # in place, versioned
    assert float(env._opp_s[0]) == 120 * env.dl + 3.0 * env.delta_t + 3.0 * env.delta_t
    assert int(env.opponent_path_indices()[-1, 2]) == path.shape[0] - 1      # held at the end of the course
    inside = torch.cat([env._opp_table[0, 1, :2], torch.zeros(2)]).view(1, 1, 4)
    assert float(env.opponent_hits(inside)) == 1.0 and float(env.collision_check(inside)) >= 1.0
    env.set_opponents([10], [1.0], 0.5, weight=[3.0])
    assert float(env.predict_opponents()[0, 0, 3]) == 3.0
    with pytest.raises(ValueError):
        env.set_opponents(list(range(9)), [1.0] * 9, 0.5)
    env.set_opponents([], [], 0.0)
    assert env.predict_opponents().shape == (T, 0, 4)


def test_controller_cost_equals_the_restatement():
    import torch

    from envs.racing_opponents import opponent_racing_controller

    T, t = 8, 3
    env = _env(T)
    ctrl = opponent_racing_controller(env, device=torch.device("cpu"), horizon=T, num_samples=64, mppi_cls=lambda **kw: None)
    ctrl.set_cost_map(env._obstacle_map, env._lane_map)
    x0 = R.start_pose(env.reset().numpy())
    ref = R.window(env.racing_center_path_np, x0, T)
    ctrl.set_reference(ref)
    table = R.case("overlap2", T, x0)[0]
    env._opp_table = torch.from_numpy(table.copy())
    spec = type(ctrl).cost_function.__mppi_native__.provider(ctrl)
    assert spec["discs"]["table"] is env._opp_table and spec["discs"]["version"] == env._opp_version and len(spec["params"]) == 17
    grids = tuple((np.ascontiguousarray(g.cells, np.uint8), float(g.cell_size), float(g.origin[0]), float(g.origin[1]))
                  for g in spec["maps"])
    rng = np.random.default_rng(1)
    cen = table[t, 0, :2]
    s = np.concatenate([cen + rng.uniform(-0.6, 0.6, (300, 2)), rng.uniform(-3, 3, (300, 1)), rng.uniform(0, 8, (300, 1))], 1).astype(f32)
    u, pu = R.actions(2, 300, 1)[:, 0], R.actions(3, 300, 1)[:, 0]
    got = ctrl.cost_function(torch.from_numpy(s), torch.from_numpy(u), {"t": t, "prev_action": torch.from_numpy(pu)}).numpy()
    pen, hit = R.penalty(table[t], 2, s[:, 0], s[:, 1])
    base = R.base_cost(f32(spec["params"]), grids, R.ref_rows(ref)[t], s, u, pu)
    assert 0.05 < hit.any(1).mean() < 0.95
    # torch's sum(dim=1) of two squares and its sin / cos of the reference yaw are one rounding each like the restatement's;
    # the disc part is exact: the difference of the two costs is the penalty, 0 or 2 x 2500 (each within an ulp of the cost)
    assert np.allclose(got, (base + pen).astype(f32), rtol=1e-6, atol=0.0)
    plain = got - pen
    assert np.allclose(plain, base, rtol=1e-6)


def test_tags_and_untagged_lambdas():
    import torch

    from envs.racing_controller import racing_controller
    from envs.racing_env import RacingEnv
    from envs.racing_opponents import opponent_racing_controller
    from pi_mpc.native import resolve

    env = _env(4)
    ctrl = opponent_racing_controller(env, device=torch.device("cpu"), horizon=4, num_samples=64, mppi_cls=lambda **kw: None)
    (dt, do), (ct, co) = resolve(env.dynamics), resolve(ctrl.cost_function)
    assert (dt.model, dt.role, ct.model, ct.role) == ("racing_discs", "dynamics", "racing_discs", "cost") and do is env and co is ctrl
    assert resolve(lambda s, a: env.dynamics(s, a)) is None
    assert RacingEnv.dynamics.__mppi_native__.model == "racing"            # the parents' tags are what they were
    assert racing_controller.cost_function.__mppi_native__.model == "racing"
    from mppi_playground_amd import _capi

    assert _capi.MODEL_IDS["racing_discs"] == 10 and _capi.MODEL_DIMS["racing_discs"] == (4, 2) and _capi.ABI_VERSION == 16
