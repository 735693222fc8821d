"""The 8-state learned-dynamics models (MPPI_MODEL_MLP81 / MLP82 / MLP84; envs.MLPModel8) without a GPU: the functor text of
csrc/mppi_models.inc compiled with g++ (tests/host_emul/mlp8_emul.cpp) against the numpy restatement of tests/mlp8_ref.py,
the Python helper (envs/mlp_model.py), and the case table the GPU test shares.

  relu, math level 0: states and costs equal the fp32 restatement BIT FOR BIT (the three ids, one and two layers, residual on
    and off, a 20-wide network and the 6-state networks against their padded forms).
  tanh and math level 1: costs within mlp_ref.band of the float64 evaluation — 4 x the fp32 restatement's own distance from
    float64, per case — measured here with the host's libm as it is on the device with the GPU's.
  The same program with its own main, built with -fsanitize=address,undefined, walks the table's cases in a child process.
"""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mlp8_ref as R

f32, f64 = np.float32, np.float64
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
SRC = os.path.join(HERE, "mlp8_emul.cpp")
N_HOST = 100


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emul_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mlp8_emul") / "libmlp8_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, SRC])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def emul(emul_lib):
    def rollout(cs, fast, U, x0=None):
        N, T, dc = U.shape
        U = np.ascontiguousarray(U, f32)
        costs, S = np.empty(N, f32), np.empty((N, T + 1, 8), f32)
        tab, par = np.ascontiguousarray(cs["table"], f32), np.ascontiguousarray(cs["params"], f32)
        x = np.ascontiguousarray(cs["x0"] if x0 is None else x0, f32)
        rc = emul_lib.mlp8_emul_rollout(dc, int(fast), _p(tab), int(tab.size), cs["hidden_layers"], int(cs["activation"] == "tanh"),
                                        int(cs["residual"]), _p(par), int(par.size), _p(x), _p(U), N, T, _p(costs), _p(S))
        assert rc == 0
        return costs, S

    return rollout


def _ref(cs, U, dtype=f32, layers=None):
    return R.rollout(cs["table"], cs["params"], cs["hidden_layers"], cs["activation"], cs["residual"], cs["x0"], U, dtype, layers)


def _own_layers(cs):
    Ws, bs = cs["Ws"], cs["bs"]
    if cs["hidden_layers"] == 2:
        return (Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2])
    return (Ws[0], bs[0], np.zeros((0, 0), f32), np.zeros(0, f32), Ws[1], bs[1])


RELU = [c[0] for c in R.CASES if c[3] == "relu"]
TANH = [c[0] for c in R.CASES if c[3] == "tanh"]
NARROW = [c[0] for c in R.CASES if c[5] != R.H or c[6] != R.DS]


# ------------------------------------------------------------------------------ the table
def test_table_covers_the_shapes(emul_lib):
    seen = {(dc, hl, act, res) for _, dc, hl, act, res, w, ds in R.CASES if w == R.H and ds == R.DS}
    assert seen == {(dc, hl, act, res) for dc in (1, 2, 4) for hl in (1, 2) for act in ("relu", "tanh") for res in (False, True)}
    assert [c[5] for c in R.CASES if c[5] != R.H] == [20]
    assert sorted(c[1] for c in R.CASES if c[6] == 6) == [1, 2, 4] and all(c[6] in (6, 8) for c in R.CASES)
    assert R.HORIZONS == {1: (1, 4, 5, 8, 9), 2: (1, 2, 3, 7, 8), 4: (1, 2, 3, 4, 5, 9)} and R.SAMPLES == (64, 100, 4160)
    assert [R.n_floats(dc) for dc in (1, 2, 4)] == [1640, 1672, 1736]
    from mppi_playground_amd import _capi

    for dc in (1, 2, 4):  # the header's sizes, counts and ids are the Python side's
        assert emul_lib.mlp8_emul_table_floats(dc) == R.n_floats(dc)
        assert emul_lib.mlp8_emul_param_count(dc) == 16 + dc
        assert emul_lib.mlp8_emul_model_id(dc) == _capi.MODEL_IDS[f"mlp8{dc}"] == {1: 13, 2: 14, 4: 15}[dc]
        assert _capi.MODEL_DIMS[f"mlp8{dc}"] == (8, dc)
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


@pytest.mark.parametrize("name", NARROW)
def test_narrow_network_equals_its_padded_form(emul, name):
    """A 20-wide network and the 6-state networks: the table's zero rows, columns and biases change no bit — the network's own
    layers from its own 6 (or 8) states, the padded table in numpy and the functor agree; components 6 and 7 stay zero."""
    cs = R.case(name)
    ds, dc = cs["ds"], cs["dc"]
    assert cs["Ws"][0].shape == (cs["width"], ds + dc) and cs["Ws"][-1].shape == (ds, cs["width"])
    U = R.actions(3, N_HOST, R.HORIZONS[dc][-1], dc)
    narrow = _ref(cs, U, layers=_own_layers(cs))
    padded = _ref(cs, U)
    got = [padded]
    if cs["activation"] == "relu":  # (the functor's tanh is the host libm's, numpy's may differ in the last bit)
        got.append(emul(cs, 0, U)[:2])
    for g in got:
        assert np.array_equal(g[0].view(np.uint32), narrow[0].view(np.uint32)), name
        assert np.array_equal(np.ascontiguousarray(g[1][:, :, :ds]).view(np.uint32), narrow[1].view(np.uint32)), name
        assert not g[1][:, :, ds:].any(), f"{name}: a padded component moved"


def test_six_state_model_equals_its_explicitly_padded_form():
    """MLPModel8 around a 6-state network against MLPModel8 around the same network written out with 8 states (zero rows and
    columns by hand): the same table, and the torch callables return the same bits."""
    import torch

    from envs import MLPModel8

    cs = R.case("mlp82_tanh_2l_res_s6")
    Ws, bs, P = cs["Ws"], cs["bs"], cs["params"]
    m6 = MLPModel8(Ws, bs, activation="tanh", residual=True, goal=P[:6], q=P[8:14], r=P[16:])
    W1 = np.zeros((32, 10), f32)
    W1[:, :6], W1[:, 8:] = Ws[0][:, :6], Ws[0][:, 6:]
    W3, b3 = np.zeros((8, 32), f32), np.zeros(8, f32)
    W3[:6], b3[:6] = Ws[2], bs[2]
    m8 = MLPModel8([W1, Ws[1], W3], [bs[0], bs[1], b3], activation="tanh", residual=True, goal=P[:8], q=P[8:16], r=P[16:])
    assert (m6.dim_state_model, m8.dim_state_model, m6.dim_state, m8.dim_state) == (6, 8, 8, 8)
    assert np.array_equal(m6.table, m8.table) and np.array_equal(m6.table, cs["table"]) and m6.table.size == 1672
    assert m6.native_inputs()["params"] == m8.native_inputs()["params"] == [float(v) for v in P]
    U = torch.from_numpy(R.actions(4, 50, 3, 2))
    s6 = m6.pad_state(torch.from_numpy(np.broadcast_to(cs["x0"][:6], (50, 6)).copy()))
    s8 = torch.from_numpy(np.broadcast_to(cs["x0"], (50, 8)).copy())
    assert torch.equal(s6, s8) and s6.shape == (50, 8)
    for t in range(3):
        assert torch.equal(m6.cost(s6, U[:, t], {}), m8.cost(s8, U[:, t], {}))
        s6, s8 = m6.dynamics(s6, U[:, t]), m8.dynamics(s8, U[:, t])
        assert torch.equal(s6, s8) and not s6[:, 6:].any()


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
    print(f"[mlp8] host {name} math {fast}: ratio {err.max() / max(yard, 1e-300):.2f} of the fp32 band {yard:.3g} "
          f"(smallest limit {limit.min():.3g})")
    assert np.all(err <= limit), f"{name} math {fast}: {err.max():.3g} > {limit[np.argmax(err - limit)]:.3g}"


# ------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_passes_the_sanitizers(emul, tmp_path):
    exe = str(tmp_path / "mlp8_emul_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-DMLP8_EMUL_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    want, blob = [], bytearray()
    for name in [c[0] for c in R.CASES]:
        cs = R.case(name)
        for fast in (0, 1):
            T = R.HORIZONS[cs["dc"]][-1]
            U = R.actions(5, 64, T, cs["dc"])
            hd = np.array([cs["dc"], fast, cs["hidden_layers"], cs["activation"] == "tanh", cs["residual"], 64, T,
                           cs["table"].size], np.int32)
            assert cs["table"].size == R.n_floats(cs["dc"]) and cs["params"].size == 16 + cs["dc"] and cs["x0"].size == 8
            blob += hd.tobytes() + cs["table"].tobytes() + cs["params"].tobytes() + cs["x0"].tobytes() + U.tobytes()
            want.append(emul(cs, fast, U)[0])
    (tmp_path / "cases.bin").write_bytes(bytes(blob))
    out = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "costs.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    assert f"{2 * len(R.CASES)} cases" in out.stdout
    got = np.fromfile(str(tmp_path / "costs.bin"), f32)
    # (the -O1 build and the -O2 library round every operation alike: contraction is off in both)
    assert np.array_equal(got.view(np.uint32), np.concatenate(want).view(np.uint32))
    assert np.all(np.isfinite(got))  # (a read past the 16 + dc parameters would have met the NaN behind them)
    out = subprocess.run([exe], capture_output=True, text=True)  # generated batches of every flag combination
    assert out.returncode == 0 and "48 runs" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------ the Python helper
def _module(dc, hidden, act, width=32, ds=8, seed=0):
    import torch

    torch.manual_seed(seed)
    A = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh}[act]
    mods = [torch.nn.Linear(ds + dc, width), A()]
    if hidden == 2:
        mods += [torch.nn.Linear(width, width), A()]
    return torch.nn.Sequential(*mods, torch.nn.Linear(width, ds))


def test_from_module_produces_the_documented_layout():
    from envs import MLPModel, MLPModel8

    assert issubclass(MLPModel8, MLPModel) and (MLPModel.DS, MLPModel8.DS) == (4, 8)
    net = _module(4, 2, "tanh", width=20, ds=6)
    goal, q, r = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [0.5, 0.25, 2.0, 1.0, 1.5, 3.0], [0.1, 0.2, 0.3, 0.4]
    m = MLPModel8.from_module(net, residual=False, goal=goal, q=q, r=r)
    assert (m.model_name, m.hidden_layers, m.activation, m.residual, m.dim_state) == ("mlp84", 2, "tanh", False, 8)
    W1, b1, W2, b2, W3, b3 = R.unpack(m.table, 4)
    lin = [l for l in net if hasattr(l, "weight")]
    w = [l.weight.detach().numpy() for l in lin]
    b = [l.bias.detach().numpy() for l in lin]
    assert np.array_equal(W1[:20, :6], w[0][:, :6]) and np.array_equal(W1[:20, 8:], w[0][:, 6:])  # controls behind 8 states
    assert not W1[:, 6:8].any() and not W1[20:].any() and np.array_equal(b1[:20], b[0]) and not b1[20:].any()
    assert np.array_equal(W2[:20, :20], w[1]) and not W2[20:].any() and not W2[:, 20:].any() and np.array_equal(b2[:20], b[1])
    assert np.array_equal(W3[:6, :20], w[2]) and not W3[6:].any() and not W3[:, 20:].any()
    assert np.array_equal(b3, np.append(b[2], f32([0, 0])))
    assert np.array_equal(m.table, R.pack(w, b, 4))
    sp = m.native_inputs()
    assert sp["params"] == goal + [0.0, 0.0] + q + [0.0, 0.0] + [float(f32(v)) for v in r] and len(sp["params"]) == 20
    assert m.goal.shape == (8,) and m.q.shape == (8,) and m.r.shape == (4,)
    assert sp["mlp"]["version"] == 0 and sp["mlp"]["table"].size == 1736
    m.update_weights(w, b)
    assert m.native_inputs()["mlp"]["version"] == 1
    for dc, n in ((1, 1640), (2, 1672), (4, 1736)):
        one = MLPModel8.from_module(_module(dc, 1, "relu"))
        assert (one.model_name, one.hidden_layers, one.activation, one.residual) == (f"mlp8{dc}", 1, "relu", True)
        assert one.table.size == n and not R.unpack(one.table, dc)[2].any()
    # MLPModel is what it was: its tags, its tables, its width
    old = MLPModel.from_module(_module(2, 2, "tanh", ds=3))
    assert (old.model_name, old.dim_state, old.table.size, old.goal.shape) == ("mlp42", 4, 1412, (4,))
    assert MLPModel.from_module(_module(1, 1, "relu", ds=4)).model_name == "mlp41"
    x = old.pad_state([1.0, 2.0, 3.0])
    assert x.tolist() == [1.0, 2.0, 3.0, 0.0] and m.pad_state(np.ones((5, 6), f32)).shape == (5, 8)
    with pytest.raises(ValueError):
        old.pad_state(np.ones(5, f32))


def test_the_tags_resolve_by_control_width():
    from envs import MLPModel8
    from pi_mpc.native import resolve

    for dc, want in ((1, "mlp81"), (2, "mlp82"), (4, "mlp84")):
        m = MLPModel8.from_module(_module(dc, 2, "tanh", ds=6))
        (dt, do), (ct, co) = resolve(m.dynamics), resolve(m.cost)
        assert (dt.model, dt.role, ct.model, ct.role) == (want, "dynamics", want, "cost") and do is m and co is m
        assert ct.provider(co)["mlp"]["table"] is m.table
        twin = copy.deepcopy(m)
        assert type(twin) is MLPModel8 and twin is not m and np.array_equal(twin.table, m.table) and twin.table is not m.table
        assert resolve(twin.cost)[1] is twin and twin.dim_state == 8


def test_the_helpers_refuse_what_the_device_does_not_take():
    from envs import MLPEnsemble, MLPModel, MLPModel8

    z = np.zeros
    with pytest.raises(ValueError):  # nine states
        MLPModel8([z((8, 10)), z((9, 8))], [z(8), z(9)])
    with pytest.raises(ValueError):  # three controls
        MLPModel8([z((8, 11)), z((8, 8))], [z(8), z(8)])
    with pytest.raises(ValueError):  # five controls
        MLPModel8([z((8, 13)), z((8, 8))], [z(8), z(8)])
    with pytest.raises(ValueError):  # no control
        MLPModel8([z((8, 8)), z((8, 8))], [z(8), z(8)])
    with pytest.raises(ValueError):  # width above 32
        MLPModel8([z((33, 10)), z((8, 33))], [z(33), z(8)])
    with pytest.raises(ValueError):  # three hidden layers
        MLPModel8([z((8, 10)), z((8, 8)), z((8, 8)), z((8, 8))], [z(8), z(8), z(8), z(8)])
    for bad_value in (np.nan, np.inf):
        bad = z((8, 10))
        bad[3, 9] = bad_value
        with pytest.raises(ValueError):
            MLPModel8([bad, z((8, 8))], [z(8), z(8)])
    with pytest.raises(ValueError):  # goal of the wrong length
        MLPModel8([z((8, 10)), z((8, 8))], [z(8), z(8)], goal=[0.0] * 4)
    m = MLPModel8([z((8, 10)), z((8, 8))], [z(8), z(8)])
    for Ws, bs in (([z((8, 12)), z((8, 8))], [z(8), z(8)]),            # another control width
                   ([z((8, 8)), z((6, 8))], [z(8), z(6)]),             # another state width (6 + 2)
                   ([z((8, 10)), z((8, 8)), z((8, 8))], [z(8)] * 3)):  # another number of layers
        with pytest.raises(ValueError):
            m.update_weights(Ws, bs)
    m.update_weights([z((16, 10)), z((8, 16))], [z(16), z(8)])  # (another hidden width is the same table)
    # MLPModel still takes four states and one or two controls
    with pytest.raises(ValueError):
        MLPModel([z((8, 6)), z((5, 8))], [z(8), z(5)])
    with pytest.raises(ValueError):
        MLPModel([z((8, 7)), z((4, 8))], [z(8), z(4)])
    with pytest.raises(ValueError):  # (four controls are MLPModel8's)
        MLPModel([z((8, 8)), z((4, 8))], [z(8), z(4)])
    # an ensemble is of one class
    a4 = MLPModel([z((8, 5)), z((4, 8))], [z(8), z(4)])
    a8 = MLPModel8([z((8, 5)), z((4, 8))], [z(8), z(4)])
    with pytest.raises(ValueError, match="one class"):
        MLPEnsemble([a4, a8])
    with pytest.raises(ValueError, match="one class"):
        MLPEnsemble([a8, a4])
    ens = MLPEnsemble([a8, copy.deepcopy(a8)])
    assert (ens.model_name, ens.dim_state, ens.tables.shape) == ("mlp81", 8, (2, 1640))
    assert MLPEnsemble([a4, copy.deepcopy(a4)]).model_name == "mlp41"


@pytest.mark.parametrize("name", [c[0] for c in R.CASES if c[2] == 2 or c[6] == 6])
def test_torch_callables_agree_with_numpy(name):
    """The callables on the CPU against float64 numpy (within the fp32 restatement's band), and — relu — equal to the fp32
    restatement bit for bit: the same operations in the same order."""
    import torch

    from envs import MLPModel8

    cs = R.case(name)
    ds, dc, P = cs["ds"], cs["dc"], cs["params"]
    m = MLPModel8([w.copy() for w in cs["Ws"]], cs["bs"], activation=cs["activation"], residual=cs["residual"], goal=P[:ds],
                  q=P[8:8 + ds], r=P[16:])
    assert np.array_equal(m.table, cs["table"]) and m.model_name == cs["model"]
    assert np.array_equal(f32(m.native_inputs()["params"]), P)
    T, N = 6, 50
    U = R.actions(2, N, T, dc)
    s = m.pad_state(torch.from_numpy(np.broadcast_to(cs["x0"][:ds], (N, ds)).copy()))
    acc = np.zeros(N, f64)
    S = [s.numpy().copy()]
    for t in range(T):
        u = torch.from_numpy(U[:, t])
        acc += m.cost(s, u, {}).numpy().astype(f64)
        s = m.dynamics(s, u)
        S.append(s.numpy().copy())
    acc += m.cost(s, torch.zeros(N, dc), {}).numpy().astype(f64)
    c, S = acc.astype(f32), np.stack(S, 1)
    c32, S32, mag = _ref(cs, U)
    c64, S64, _ = _ref(cs, U, f64)
    limit, _ = R.band(c32, c64, mag)
    assert np.all(np.abs(c.astype(f64) - c64) <= limit)
    assert np.allclose(S, S64, rtol=0, atol=1e-5)
    if cs["activation"] == "relu":
        assert np.array_equal(S.view(np.uint32), S32.view(np.uint32))
        assert np.array_equal(c.view(np.uint32), c32.view(np.uint32))
    assert not S[:, :, ds:].any()  # the padded components stay zero


def test_cost_parameters_change_for_callables_and_device_alike():
    import torch

    from envs import MLPModel8

    cs = R.case("mlp84_relu_1l_abs")
    m = MLPModel8(cs["Ws"], cs["bs"], activation="relu", residual=False, goal=[0.0] * 8, q=[1.0] * 8, r=[0.0] * 4)
    s, u = torch.ones(3, 8), torch.zeros(3, 4)
    assert torch.equal(m.cost(s, u, {}), torch.full((3,), 8.0))
    with pytest.raises(ValueError):  # (the arrays are read-only: nothing can move them behind the callables' back)
        m.goal[0] = 1.0
    m.set_cost(goal=[1.0] * 7 + [0.0], r=[2.0, 0.0, 0.0, 1.0])
    assert torch.equal(m.cost(s, u + 1, {}), torch.full((3,), 4.0))
    assert m.native_inputs()["params"] == [1.0] * 7 + [0.0] + [1.0] * 8 + [2.0, 0.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        m.set_cost(q=[1.0, 2.0, 3.0, 4.0])
