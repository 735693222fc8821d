"""The learned-dynamics models (MPPI_MODEL_MLP41 / MLP42) without a GPU: the functor text of csrc/mppi_models.inc compiled
with g++ (tests/host_emul/mlp_emul.cpp) against the numpy restatement of tests/mlp_ref.py, the Python helper
(envs/mlp_model.py), and the case table the GPU test shares.

  relu, math level 0: states and costs equal the fp32 restatement BIT FOR BIT (both ids, one and two layers, residual on
    and off, a 20-wide network against its padded form).
  tanh and math level 1: costs within mlp_ref.band of the float64 evaluation — 4 x the fp32 restatement's own distance from
    float64, per case — measured here with the host's libm as it is on the device with the GPU's.
  The same program with its own main, built with -fsanitize=address,undefined, walks the table's cases.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mlp_ref as R

f32, f64 = np.float32, np.float64
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
SRC = os.path.join(HERE, "mlp_emul.cpp")
N_HOST, T_HOST = 100, 9


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mlp_emul") / "libmlp_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, SRC])
    lib = C.CDLL(so)

    def rollout(cs, fast, U, x0=R.X0):
        N, T, dc = U.shape
        U = np.ascontiguousarray(U, f32)
        costs, S = np.empty(N, f32), np.empty((N, T + 1, 4), f32)
        tab, par, x = np.ascontiguousarray(cs["table"], f32), np.ascontiguousarray(cs["params"], f32), np.ascontiguousarray(x0, f32)
        rc = lib.mlp_emul_rollout(dc, int(fast), _p(tab), int(tab.size), cs["hidden_layers"], int(cs["activation"] == "tanh"),
                                  int(cs["residual"]), _p(par), int(par.size), _p(x), _p(U), N, T, _p(costs), _p(S))
        assert rc == 0
        return costs, S

    return rollout


def _ref(cs, U, dtype=f32, layers=None):
    return R.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], R.X0, U, dtype, layers)


RELU = [c[0] for c in R.CASES if c[3] == "relu"]
TANH = [c[0] for c in R.CASES if c[3] == "tanh"]


# ------------------------------------------------------------------------------ the table
def test_table_covers_the_shapes():
    seen = {(dc, hl, act, res) for _, dc, hl, act, res, w in R.CASES if w == R.H}
    assert seen == {(dc, hl, act, res) for dc in (1, 2) for hl in (1, 2) for act in ("relu", "tanh") for res in (False, True)}
    assert {(c[3], c[5]) for c in R.CASES if c[5] != R.H} == {("relu", 20), ("tanh", 20)}
    assert R.HORIZONS == {1: (1, 4, 5, 8, 9), 2: (1, 2, 3, 7, 8)} and R.SAMPLES == (64, 100, 4160)
    assert R.n_floats(1) == 1380 and R.n_floats(2) == 1412
    for name in TANH:  # contractions: spectral norms <= 0.9; residual only with a 0.05 output layer
        cs = R.case(name)
        norms = [np.linalg.norm(W.astype(f64), 2) for W in cs["Ws"]]
        assert max(norms[:-1]) <= 0.9 * (1 + 1e-6), name
        assert norms[-1] <= (0.05 * 0.9 if cs["residual"] else 0.9) * (1 + 1e-6), name


# ------------------------------------------------------------------------------ relu, level 0: bit for bit
@pytest.mark.parametrize("name", RELU)
def test_relu_level0_equals_the_fp32_restatement(emul, name):
    cs = R.case(name)
    for T in R.HORIZONS[cs["dc"]]:
        U = R.actions(7 + T, N_HOST, T, cs["dc"])
        c, S = emul(cs, 0, U)
        c32, S32, _ = _ref(cs, U)
        assert np.array_equal(S.view(np.uint32), S32.view(np.uint32)), f"{name} T={T}: states (the step)"
        assert np.array_equal(c.view(np.uint32), c32.view(np.uint32)), f"{name} T={T}: costs"
        assert np.any(S[:, -1] != S[:, 0]) and np.all(np.isfinite(c))


def test_narrow_network_equals_its_padded_form(emul):
    cs = R.case("mlp41_relu_2l_res_w20")
    Ws, bs = cs["Ws"], cs["bs"]
    assert Ws[0].shape == (20, 5) and Ws[1].shape == (20, 20) and Ws[2].shape == (4, 20)
    U = R.actions(3, N_HOST, T_HOST, 1)
    narrow = _ref(cs, U, layers=(Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2]))
    padded = _ref(cs, U)
    c, S = emul(cs, 0, U)
    for got in (padded[0], c):
        assert np.array_equal(got.view(np.uint32), narrow[0].view(np.uint32))
    assert np.array_equal(S.view(np.uint32), narrow[1].view(np.uint32))


# ------------------------------------------------------------------------------ tanh and level 1: the band
# (relu at level 0 is held bit for bit above)
@pytest.mark.parametrize("name,fast", [(c[0], fast) for c in R.CASES for fast in (0, 1) if c[3] == "tanh" or fast])
def test_costs_within_the_band_of_float64(emul, name, fast):
    cs = R.case(name)
    T = R.HORIZONS[cs["dc"]][-1]
    U = R.actions(11, N_HOST, T, cs["dc"])
    c, _ = emul(cs, fast, U)
    c32, _, mag = _ref(cs, U)
    c64, _, _ = _ref(cs, U, f64)
    limit, yard = R.band(c32, c64, mag)
    err = np.abs(c.astype(f64) - c64)
    print(f"[mlp] host {name} math {fast}: ratio {err.max() / max(yard, 1e-300):.2f} of the fp32 band {yard:.3g} "
          f"(smallest limit {limit.min():.3g})")
    assert np.all(err <= limit), f"{name} math {fast}: {err.max():.3g} > {limit[np.argmax(err - limit)]:.3g}"


# ------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_passes_the_sanitizers(emul, tmp_path):
    exe = str(tmp_path / "mlp_emul_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-DMLP_EMUL_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    want, blob = [], bytearray()
    for name in [c[0] for c in R.CASES]:
        cs = R.case(name)
        for fast in (0, 1):
            T = R.HORIZONS[cs["dc"]][-1]
            U = R.actions(5, 64, T, cs["dc"])
            hd = np.array([cs["dc"], fast, cs["hidden_layers"], cs["activation"] == "tanh", cs["residual"], 64, T,
                           cs["table"].size], np.int32)
            blob += hd.tobytes() + cs["table"].tobytes() + cs["params"].tobytes() + R.X0.tobytes() + U.tobytes()
            want.append(emul(cs, fast, U)[0])
    (tmp_path / "cases.bin").write_bytes(bytes(blob))
    out = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "costs.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    got = np.fromfile(str(tmp_path / "costs.bin"), f32)
    # (the -O1 build and the -O2 library round every operation alike: contraction is off in both)
    assert np.array_equal(got.view(np.uint32), np.concatenate(want).view(np.uint32))
    out = subprocess.run([exe], capture_output=True, text=True)  # generated batches of every flag combination
    assert out.returncode == 0 and "32 runs" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------ the Python helper
def _module(dc, hidden, act, width=32, ds=4, seed=0):
    import torch

    torch.manual_seed(seed)
    A = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh}[act]
    mods = [torch.nn.Linear(ds + dc, width), A()]
    if hidden == 2:
        mods += [torch.nn.Linear(width, width), A()]
    return torch.nn.Sequential(*mods, torch.nn.Linear(width, ds))


def test_from_module_produces_the_documented_layout():
    from envs import MLPModel

    net = _module(2, 2, "tanh", width=20, ds=3)
    m = MLPModel.from_module(net, residual=False, goal=[1.0, 2.0, 3.0], q=[0.5, 0.25, 2.0], r=[0.1, 0.2])
    assert (m.model_name, m.hidden_layers, m.activation, m.residual) == ("mlp42", 2, "tanh", False)
    W1, b1, W2, b2, W3, b3 = R.unpack(m.table, 2)
    lin = [l for l in net if hasattr(l, "weight")]
    w = [l.weight.detach().numpy() for l in lin]
    b = [l.bias.detach().numpy() for l in lin]
    assert np.array_equal(W1[:20, :3], w[0][:, :3]) and np.array_equal(W1[:20, 4:], w[0][:, 3:])  # controls behind 4 states
    assert not W1[:, 3].any() and not W1[20:].any() and np.array_equal(b1[:20], b[0]) and not b1[20:].any()
    assert np.array_equal(W2[:20, :20], w[1]) and not W2[20:].any() and not W2[:, 20:].any() and np.array_equal(b2[:20], b[1])
    assert np.array_equal(W3[:3, :20], w[2]) and not W3[3].any() and not W3[:, 20:].any()
    assert np.array_equal(b3, np.append(b[2], f32(0)))
    sp = m.native_inputs()
    assert sp["params"] == [1.0, 2.0, 3.0, 0.0, 0.5, 0.25, 2.0, 0.0, f32(0.1), f32(0.2)]
    assert sp["mlp"]["version"] == 0 and sp["mlp"]["table"].size == 1412
    m.update_weights(w, b)
    assert m.native_inputs()["mlp"]["version"] == 1
    one = MLPModel.from_module(_module(1, 1, "relu"))
    assert (one.model_name, one.hidden_layers, one.activation, one.residual) == ("mlp41", 1, "relu", True)
    assert one.table.size == 1380 and not R.unpack(one.table, 1)[2].any()


def test_the_tags_resolve_by_control_width():
    import copy

    from envs import MLPModel
    from pi_mpc.native import resolve

    for dc, want in ((1, "mlp41"), (2, "mlp42")):
        m = MLPModel.from_module(_module(dc, 2, "tanh"))
        (dt, do), (ct, co) = resolve(m.dynamics), resolve(m.cost)
        assert (dt.model, dt.role, ct.model, ct.role) == (want, "dynamics", want, "cost") and do is m and co is m
        assert ct.provider(co)["mlp"]["table"] is m.table
        twin = copy.deepcopy(m)
        assert twin is not m and np.array_equal(twin.table, m.table) and twin.table is not m.table
        assert resolve(twin.cost)[1] is twin


def test_the_helper_refuses_what_the_device_does_not_take():
    import torch

    from envs import MLPModel

    z = np.zeros
    with pytest.raises(ValueError):  # three hidden layers
        MLPModel([z((8, 5)), z((8, 8)), z((8, 8)), z((4, 8))], [z(8), z(8), z(8), z(4)])
    with pytest.raises(ValueError):  # width above 32
        MLPModel([z((33, 5)), z((4, 33))], [z(33), z(4)])
    with pytest.raises(ValueError):  # state wider than 4
        MLPModel([z((8, 6)), z((5, 8))], [z(8), z(5)])
    with pytest.raises(ValueError):  # three controls
        MLPModel([z((8, 7)), z((4, 8))], [z(8), z(4)])
    with pytest.raises(ValueError):  # no control
        MLPModel([z((8, 4)), z((4, 8))], [z(8), z(4)])
    with pytest.raises(ValueError):
        MLPModel([z((8, 5)), z((4, 8))], [z(8), z(4)], activation="gelu")
    bad = z((8, 5))
    bad[0, 0] = np.nan
    with pytest.raises(ValueError):
        MLPModel([bad, z((4, 8))], [z(8), z(4)])
    with pytest.raises(ValueError):
        MLPModel.from_module(torch.nn.Sequential(torch.nn.Linear(5, 8), torch.nn.Sigmoid(), torch.nn.Linear(8, 4)))
    m = MLPModel([z((8, 5)), z((4, 8))], [z(8), z(4)])
    with pytest.raises(ValueError):  # another control width
        m.update_weights([z((8, 6)), z((4, 8))], [z(8), z(4)])


@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp42_tanh_2l_abs", "mlp41_tanh_1l_res", "mlp42_relu_1l_abs_unpadded"])
def test_torch_callables_agree_with_numpy(name):
    """The callables on the CPU against float64 numpy (within the fp32 restatement's band), and — relu — equal to the fp32
    restatement bit for bit: the same operations in the same order."""
    import torch

    from envs import MLPModel

    unpadded = name.endswith("_unpadded")
    cs = R.case("mlp41_relu_2l_res_w20" if unpadded else name)
    if unpadded:  # a 3-state model with narrow layers: the helper pads the weights, the caller the state
        rng = np.random.default_rng(5)
        Ws = [R._spectral_scale(rng.standard_normal(s), 0.9) for s in ((20, 4), (20, 20), (3, 20))]
        bs = [(0.1 * rng.standard_normal(n)).astype(f32) for n in (20, 20, 3)]
        m = MLPModel(Ws, bs, activation="relu", residual=True, goal=cs["params"][:3], q=cs["params"][4:7], r=cs["params"][8:9])
        cs = dict(cs, table=m.table, params=f32(m.native_inputs()["params"]))
        x0 = f32([0.3, -0.2, 0.5, 0.0])
    else:
        W = [w.copy() for w in cs["Ws"]]
        m = MLPModel(W, cs["bs"], activation=cs["activation"], residual=cs["residual"], goal=cs["params"][:4],
                     q=cs["params"][4:8], r=cs["params"][8:])
        assert np.array_equal(m.table, cs["table"])
        x0 = R.X0
    dc, T, N = cs["dc"], 6, 50
    U = R.actions(2, N, T, dc)
    s = torch.from_numpy(np.broadcast_to(x0, (N, 4)).copy())
    acc = np.zeros(N, f64)
    S = [s.numpy().copy()]
    for t in range(T):
        u = torch.from_numpy(U[:, t])
        acc += m.cost(s, u, {}).numpy().astype(f64)
        s = m.dynamics(s, u)
        S.append(s.numpy().copy())
    acc += m.cost(s, torch.zeros(N, dc), {}).numpy().astype(f64)
    c = acc.astype(f32)
    c32, S32, mag = R.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], x0, U)
    c64, S64, _ = R.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], x0, U, f64)
    limit, _ = R.band(c32, c64, mag)
    assert np.all(np.abs(c.astype(f64) - c64) <= limit)
    assert np.allclose(np.stack(S, 1), S64, rtol=0, atol=1e-5)
    if cs["activation"] == "relu":
        assert np.array_equal(np.stack(S, 1).view(np.uint32), S32.view(np.uint32))
        assert np.array_equal(c.view(np.uint32), c32.view(np.uint32))
    if unpadded:
        assert not np.stack(S, 1)[:, :, 3].any()  # the padded component stays zero


def test_cost_parameters_change_for_callables_and_device_alike():
    import torch

    from envs import MLPModel

    cs = R.case("mlp41_relu_1l_abs")
    m = MLPModel(cs["Ws"], cs["bs"], activation="relu", residual=False, goal=[0.0] * 4, q=[1.0] * 4, r=[0.0])
    s, u = torch.ones(3, 4), torch.zeros(3, 1)
    assert torch.equal(m.cost(s, u, {}), torch.full((3,), 4.0))
    with pytest.raises(ValueError):  # (the arrays are read-only: nothing can move them behind the callables' back)
        m.goal[0] = 1.0
    m.set_cost(goal=[1.0, 1.0, 1.0, 0.0], r=[2.0])
    assert torch.equal(m.cost(s, u + 1, {}), torch.full((3,), 3.0))
    assert m.native_inputs()["params"] == [1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 2.0]
    with pytest.raises(ValueError):
        m.set_cost(q=[1.0, 2.0])
