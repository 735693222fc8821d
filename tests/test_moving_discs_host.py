"""The moving-disc model (MPPI_MODEL_NAV2D_DISCS) without a GPU: the functor text of csrc/mppi_models.inc and
csrc/mppi_discs.hpp compiled with g++ (tests/host_emul/discs_emul.cpp) against the numpy restatement of tests/discs_ref.py,
the claims of the case table the GPU test shares, and envs.MovingObstacleNav2DEnv on CPU tensors.

  math level 0: states and costs equal the fp32 restatement BIT FOR BIT on every case and horizon; n = 0 and all-miss tables
    equal the plain nav2d functor bit for bit.
  math level 1: costs within 2e-6 of the cost scale of the float64 restatement for every sample the boundary rule keeps
    (discs_ref: `near`, `edge`); the disc arithmetic of that level (d2 = fma(dx, dx, dy * dy)) is spelled out, so the
    restatement with fuse=True on the functor's own states equals it bit for bit too.
  The same program with its own main, built with -fsanitize=address,undefined, walks the table's cases.
The map, the parameters and the start pose are nav2d's golden fixture (tests/golden/nav2d_env.npz).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import discs_ref as R
from helpers import nav2d_env_fixture, orc

f32, f64 = np.float32, np.float64
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
SRC = os.path.join(HERE, "discs_emul.cpp")
N_HOST = 100
ALL_T = R.HORIZONS + (R.T_LONG,)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def world():
    e = nav2d_env_fixture()
    grid = (np.ascontiguousarray(e["map"], np.uint8), float(e["cell"]), float(e["origin"][0]), float(e["origin"][1]))
    return f32(orc.nav2d_params()), grid


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("discs_emul") / "libdiscs_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.discs_emul_rollout.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                       C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    P, grid = world()

    def rollout(table, x0, U, fast=0, plain=0):
        N, T, _ = U.shape
        U = np.ascontiguousarray(U, f32)
        tab8 = np.ascontiguousarray(R.padded(table))
        costs, S = np.empty(N, f32), np.empty((N, T + 1, 3), f32)
        x = np.ascontiguousarray(x0, f32)
        rc = lib.discs_emul_rollout(int(fast), int(plain), _p(P), _p(grid[0]), grid[0].shape[0], grid[0].shape[1], grid[1], grid[2],
                                    grid[3], _p(tab8), tab8.shape[0], table.shape[1], _p(x), _p(U), N, T, _p(costs), _p(S))
        assert rc == 0
        return costs, S

    rollout.krow = lib.discs_emul_krow()
    return rollout


# ------------------------------------------------------------------------------ the table's claims
def test_table_claims():
    P, grid = world()
    assert set(R.CASES) >= {"step0", "stage_last", "terminal", "slot7", "overlap8", "weights8", "n0", "n1", "n3", "n8", "x0out"}
    assert R.SAMPLES == (64, 100, 4160) and R.HORIZONS == (1, 2, 3, 7, 8) and R.T_LONG == 25
    assert {R.case(n, 8)[0].shape[1] for n in ("n0", "n1", "n3", "n8")} == {0, 1, 3, 8}
    assert not (P[5] <= R.X0_OUT[0] <= P[6]) and P[5] <= R.X0[0] <= P[6]  # the x0out case starts outside the position clamp
    pad = R.padded(R.case("n3", 7)[0])
    assert pad.shape == (7, 8, 4) and np.all(pad[:, 3:, 2] == -1.0) and np.all(pad[:, 3:, 3] == 0.0) and np.all(pad[:, 3:, :2] == 0.0)
    assert len(set(np.float32(sum(R.WEIGHTS8[list(p)], f32(0))) for p in ([0, 1, 2, 3, 4, 5, 6, 7], [7, 6, 5, 4, 3, 2, 1, 0]))) == 2
    for T in ALL_T:
        U = R.actions(100 + T, 512, T)
        for name in R.CASES:
            table, x0 = R.case(name, T)
            r = [np.sqrt(table[..., 2].astype(f64))] if table.size else []
            assert all(np.all(((x >= 0.15 - 1e-6) & (x <= 0.45 + 1e-6)) | (table[..., 0] == R.FAR[0])) for x in r), name
            if table.shape[0] > 1 and table.size:  # speeds <= 1 m/s between the rows of a moving disc
                mv = np.hypot(*(np.diff(table[..., :2].astype(f64), axis=0).transpose(2, 0, 1))) / 0.1
                assert np.all((mv <= 1.0 + 1e-4) | (np.abs(np.diff(table[..., 0], axis=0)) > 30)), name
            r64 = R.rollout(P, grid, table, x0, U, f64)
            hit = r64["hit"]
            left = int(r64["near"].sum())
            share = float(hit.any(axis=(1, 2)).mean()) if hit.size else 0.0
            print(f"[discs] table {name} T{T}: hit share {share:.3f}, left out {left} of {len(U)} (cap {R.cap(len(U))})")
            assert left <= R.cap(len(U)), f"{name} T{T}: the boundary rule would leave out {left} samples"
            if name in R.MIXED and T >= 7:
                assert 0.05 <= share <= 0.95, f"{name} T{T}: hit share {share:.3f}"
            if name == "step0":  # row 0 only: every sample, at the start pose, nowhere else (T = 1: the terminal cost reads row 0 too)
                assert hit[:, 0].all() and not hit[:, 1:T].any() and (T == 1 or not hit[:, T].any())
            if name == "stage_last":  # samples the stage cost of step T-1 catches and the terminal cost does not
                assert (hit[:, T - 1, 0] & ~hit[:, T, 0]).mean() >= 0.05 and not hit[:, :T - 1].any()
            if name == "terminal":    # ... and the other way round: only a terminal cost that reads row T-1 sees them
                assert (hit[:, T, 0] & ~hit[:, T - 1, 0]).mean() >= 0.05 and not hit[:, :T - 1].any()
            if name == "slot7":
                assert hit[:, :, 7].any() and not hit[:, :, :7].any()
            if name == "overlap8" and T >= 7:
                assert np.all(hit.sum(2)[hit.any(2)] == 8)


def test_row_width(emul):
    assert emul.krow == R.KROW == 4 * R.MAX_DISCS


# ------------------------------------------------------------------------------ level 0: bit for bit
@pytest.mark.parametrize("name", list(R.CASES))
def test_level0_equals_the_fp32_restatement(emul, name):
    P, grid = world()
    for T in ALL_T:
        table, x0 = R.case(name, T)
        U = R.actions(7 + T, N_HOST, T)
        c, S = emul(table, x0, U)
        r32 = R.rollout(P, grid, table, x0, U)
        assert np.array_equal(bits(S), bits(r32["S"])), f"{name} T={T}: states"
        assert np.array_equal(bits(c), bits(r32["costs"])), f"{name} T={T}: costs"
        assert np.all(np.isfinite(c))
        if name in ("n0",) or not r32["hit"].any():  # nothing hit: the plain nav2d functor's cost, bit for bit
            cp, Sp = emul(table, x0, U, plain=1)
            assert np.array_equal(bits(c), bits(cp)) and np.array_equal(bits(S), bits(Sp)), f"{name} T={T}: plain nav2d"


def test_all_miss_equals_plain_nav2d(emul):
    table = np.broadcast_to(R.FAR, (8, 8, 4)).copy()
    U = R.actions(3, N_HOST, 8)
    for fast in (0, 1):
        c, S = emul(table, R.X0, U, fast=fast)
        cp, Sp = emul(table, R.X0, U, fast=fast, plain=1)
        assert np.array_equal(bits(c), bits(cp)) and np.array_equal(bits(S), bits(Sp))


def test_the_restatement_can_fail():
    """The cases tell a wrong reading of the table apart: row t + 1, slot 7 skipped, no terminal row."""
    P, grid = world()
    T = 8
    U = R.actions(5, 256, T)

    def differs(name, wrong):
        table, x0 = R.case(name, T)
        return not np.array_equal(R.rollout(P, grid, table, x0, U)["costs"], R.rollout(P, grid, wrong(table), x0, U)["costs"])

    assert differs("n3", lambda t: np.concatenate([t[1:], t[-1:]]))      # row t + 1
    assert differs("slot7", lambda t: t[:, :7])                          # slot 7 skipped
    assert differs("terminal", lambda t: np.broadcast_to(R.FAR, t.shape))  # (only the terminal cost and step T-1 read that row)
    w = R.case("weights8", T)[0]
    assert differs("weights8", lambda t: w[:, ::-1])                     # the summation order


# ------------------------------------------------------------------------------ level 1: the parity rule
@pytest.mark.parametrize("name", list(R.CASES))
def test_level1_within_the_parity_rule(emul, name):
    P, grid = world()
    for T in ALL_T:
        table, x0 = R.case(name, T)
        U = R.actions(11 + T, N_HOST, T)
        c, S = emul(table, x0, U, fast=1)
        r64 = R.rollout(P, grid, table, x0, U, f64)
        keep = ~(r64["near"] | r64["edge"])
        assert int(r64["near"].sum()) <= R.cap(N_HOST)
        err = np.abs(c.astype(f64) - r64["costs"])[keep]
        print(f"[discs] host {name} T{T} math 1: left out {int((~keep).sum())}, max err {err.max() / r64['scale']:.3g} of the scale")
        assert np.all(err <= R.PARITY * r64["scale"]), f"{name} T={T}: {err.max():.3g} against {R.PARITY * r64['scale']:.3g}"
        own = R.rollout(P, grid, table, x0, U, f32, states=S, fuse=True)  # the spelled-out FMA on the functor's own states
        assert np.array_equal(bits(c), bits(own["costs"])), f"{name} T={T}: level-1 costs on the functor's states"


# ------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_passes_the_sanitizers(emul, tmp_path):
    exe = str(tmp_path / "discs_emul_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-DDISCS_EMUL_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    P, grid = world()
    want, blob = [], bytearray()
    for name in R.CASES:
        for T in (1, 3, 8):
            for fast in (0, 1):
                table, x0 = R.case(name, T)
                U = R.actions(5, 64, T)
                hd = np.array([fast, 0, 64, T, T, table.shape[1], grid[0].shape[0], grid[0].shape[1]], np.int32)
                blob += (hd.tobytes() + P.tobytes() + f32(grid[1:]).tobytes() + grid[0].tobytes() + R.padded(table).tobytes()
                         + f32(x0).tobytes() + U.tobytes())
                want.append(emul(table, x0, U, fast=fast)[0])
    (tmp_path / "cases.bin").write_bytes(bytes(blob))
    out = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "costs.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    assert f"{len(want)} cases" in out.stdout
    got = np.fromfile(str(tmp_path / "costs.bin"), f32)
    assert np.array_equal(bits(got), bits(np.concatenate(want)))


# ------------------------------------------------------------------------------ the environment, on CPU tensors
def _env(T=8):
    import torch

    from envs import MovingObstacleNav2DEnv

    return MovingObstacleNav2DEnv(horizon=T, device=torch.device("cpu"))


def test_env_cost_function_equals_the_restatement():
    import torch

    T = 8
    env = _env(T)
    m = env._obstacle_map.grid_spec()
    grid = (np.ascontiguousarray(m.cells, np.uint8), float(m.cell_size), float(m.origin[0]), float(m.origin[1]))
    P = f32(type(env).cost_function.__mppi_native__.provider(env)["params"])
    table, _ = R.case("weights8", T)
    env._disc_table = torch.from_numpy(table.copy())
    rng = np.random.default_rng(1)
    cen = table[3, 0, :2]
    s = np.concatenate([cen + rng.uniform(-0.6, 0.6, (300, 2)), rng.uniform(-3, 3, (300, 1))], 1).astype(f32)
    got = env.cost_function(torch.from_numpy(s), torch.zeros(300, 2), {"t": 3}).numpy()
    pen, hit = R.penalty(table[3], 8, s[:, 0], s[:, 1])
    want = (R.base_cost(P, grid, s) + pen).astype(f32)
    assert 0.05 < hit.any(1).mean() < 0.95
    assert np.array_equal(bits(got), bits(want))


def test_env_prediction_is_in_place_and_versioned():
    import torch

    env = _env(5)
    assert env.predict_discs().shape == (5, 0, 4)
    pos, vel = torch.tensor([[-8.0, -8.5], [-7.0, -7.0]]), torch.tensor([[0.5, -0.5], [0.0, 1.0]])
    env.set_moving_obstacles(pos, vel, [0.3, 0.45])
    tab = env.predict_discs()
    assert tab.shape == (5, 2, 4) and tab is env._disc_table
    t = torch.arange(5, dtype=torch.float32).view(-1, 1, 1) * 0.1
    assert torch.equal(tab[:, :, :2], pos.unsqueeze(0) + vel.unsqueeze(0) * t)
    assert torch.equal(tab[:, :, 2], (torch.tensor([0.3, 0.45]) ** 2).expand(5, 2))
    assert torch.equal(tab[:, :, 3], torch.full((5, 2), env.obstacle_weight))
    v0, ptr = env._disc_version, tab.data_ptr()
    env.step(torch.tensor([1.0, 0.0]))
    assert env._disc_version > v0 and env._disc_table.data_ptr() == ptr
    assert torch.equal(env._disc_table[0, :, :2], pos + vel * 0.1)
    spec = type(env).cost_function.__mppi_native__.provider(env)
    assert spec["discs"]["table"] is env._disc_table and spec["discs"]["version"] == env._disc_version and len(spec["params"]) == 12
    env.set_moving_obstacles(pos, vel, 0.2, weight=[1.0, 2.0])
    assert torch.equal(env.predict_discs()[0, :, 3], torch.tensor([1.0, 2.0]))
    inside = torch.tensor([[[float(env._disc_pos[0, 0]), float(env._disc_pos[0, 1]), 0.0]]])
    assert float(env.collision_check(inside)) >= 1.0
    env.set_moving_obstacles(torch.zeros(0, 2), torch.zeros(0, 2), 0.0)
    assert env.predict_discs().shape == (5, 0, 4)


def test_env_refuses_more_than_eight():
    import torch

    env = _env(4)
    with pytest.raises(ValueError):
        env.set_moving_obstacles(torch.zeros(9, 2), torch.zeros(9, 2), 0.2)


def test_tags_and_untagged_lambdas():
    from envs.navigation_2d import Navigation2DEnv
    from pi_mpc.native import resolve

    env = _env(4)
    (dt, do), (ct, co) = resolve(env.dynamics), resolve(env.cost_function)
    assert (dt.model, dt.role, ct.model, ct.role) == ("nav2d_discs", "dynamics", "nav2d_discs", "cost") and do is env and co is env
    assert resolve(lambda s, a: env.dynamics(s, a)) is None
    assert Navigation2DEnv.cost_function.__mppi_native__.model == "nav2d"  # the parent's tags are what they were
