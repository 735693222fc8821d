"""The learned terminal value of the learned-dynamics models (include/mppi_hip.h: mppi_set_mlp_value; envs.MLPModel.set_value /
terminal_cost) without a GPU: the torch callable (envs/mlp_model.py) and the functor text of csrc/mppi_models.inc compiled with
g++ (tests/host_emul/mlp_value_emul.cpp) are held to the numpy restatement of tests/mlp_value_ref.py.

  relu, math level 0: bit for bit, on final states that make hidden units of BOTH signs (checked first).
  tanh and math level 1: within mlp_ref.band of float64, the measured ratio printed.
"""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import mlp_track_ref as TR
import mlp_value_ref as VR

f32, f64 = np.float32, np.float64
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul", "mlp_value_emul.cpp")
# one relu case per id (the 6-state network among them: ds < DS), and the tanh twins for the band
RELU = ["mlp41_relu_2l_res", "mlp42_relu_1l_abs", "mlp81_relu_2l_res_s6", "mlp82_relu_2l_res", "mlp84_relu_1l_abs"]
TANH = ["mlp41_tanh_2l_res", "mlp42_tanh_1l_abs", "mlp82_tanh_2l_res_s6", "mlp84_tanh_2l_res"]
# value networks: (hidden layers, width), each with relu and tanh
VALUES = [(1, 32), (2, 32), (2, 20), (1, 7)]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(name, got, want):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} differ, first {got[bad][:3]} against {want[bad][:3]}"


def model_of(cs, angular=()):
    from envs import MLPModel, MLPModel8

    P, ds, DS = cs["params"], cs["ds"], cs["DS"]
    cls = MLPModel if DS == 4 else MLPModel8
    return cls(cs["Ws"], cs["bs"], activation=cs["activation"], residual=cs["residual"], goal=P[:ds], q=P[DS:DS + ds],
               r=P[2 * DS:], angular=angular)


def value_for(cs, k, activation, scale=1.0):
    hidden, width = VALUES[k % len(VALUES)]
    return VR.make_value(k + 10 * len(cs["name"]), cs["ds"], hidden, activation, width, scale)


def pad(S, DS):
    out = np.zeros(S.shape[:-1] + (DS,), S.dtype)
    out[..., :S.shape[-1]] = S
    return out


# ------------------------------------------------------------------------------ the torch callable
@pytest.mark.parametrize("name", RELU)
def test_terminal_cost_in_torch_equals_the_restatement_bit_for_bit(name):
    cs = TR.case(name)
    T, N = cs["horizons"][-1], 100
    U = TR.actions(cs, 3, N, T)
    ref = TR.reference(cs, T)
    for k in range(len(VALUES)):
        val = value_for(cs, k, "relu")
        for replace in (False, True):
            for table, angular in ((None, ()), (ref, cs["angular"])):
                m = model_of(cs, angular)
                if table is not None:
                    m.set_reference(torch.from_numpy(table[:, :cs["ds"]].copy()), torch.from_numpy(table[:, cs["DS"]:cs["DS"] + cs["ds"]].copy()))
                m.set_value(val["Ws"], val["bs"], activation="relu", weight=0.75, replace_terminal=replace)
                c32, S, _ = VR.rollout(cs, val, U, ref=table, angular=angular, weight=0.75, replace_terminal=replace)
                sT = pad(S[:, T], cs["DS"])
                # the inputs make hidden units of both signs, in every sample
                layers = VR.unpack(VR.pack(val["Ws"], val["bs"], cs["ds"], cs["DS"]), cs["DS"])
                v, _, z1 = VR.value(layers, sT, val["hidden_layers"], "relu", want_hidden=True)
                z1 = z1[:, :val["width"]]
                assert np.all((z1 > 0).any(axis=1)) and np.all((z1 < 0).any(axis=1)), name
                st = torch.from_numpy(sT)
                same_bits(f"{name} value {k}: V", m.value_of(st).numpy(), v)
                # the whole cost through the callables, in the generic path's order of operations
                acc = np.zeros(N, f64)
                for t in range(T):
                    acc += m.cost(torch.from_numpy(pad(S[:, t], cs["DS"])), torch.from_numpy(U[:, t]), {"t": t}).numpy().astype(f64)
                quad = m.cost(st, torch.zeros(N, cs["dc"]), {"t": T - 1}).numpy()
                extra = m.terminal_cost(st, {"t": T - 1}).numpy()
                if not replace:  # quad + (weight * V): the device's terminal, bit for bit
                    same_bits(f"{name} value {k} ref {table is not None}: total", (acc + (quad + extra).astype(f64)).astype(f32), c32)
                    assert not np.array_equal(c32, VR.rollout(cs, None, U, ref=table, angular=angular)[0])
                else:            # quad + (weight * V - quad): weight * V up to the roundings of the two additions
                    wv = f32(0.75) * v
                    assert np.allclose(quad + extra, wv, rtol=0, atol=4 * 2.0 ** -24 * (np.abs(quad) + np.abs(wv)).max())
                    same_bits(f"{name} value {k}: replaced terminal", (acc + wv.astype(f64)).astype(f32), c32)


def test_terminal_cost_without_info_reads_the_last_row():
    cs = TR.case("mlp42_relu_1l_abs")
    T = 3
    ref = TR.reference(cs, T)
    m = model_of(cs)
    m.set_reference(torch.from_numpy(ref[:, :4].copy()), torch.from_numpy(ref[:, 4:8].copy()))
    val = value_for(cs, 1, "tanh")
    m.set_value(val["Ws"], val["bs"], replace_terminal=True)
    s = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (9, 4)).astype(f32))
    assert torch.equal(m.terminal_cost(s), m.terminal_cost(s, {"t": T - 1}))


# ------------------------------------------------------------------------------ table layout and padding
@pytest.mark.parametrize("name", ["mlp41_relu_2l_res", "mlp81_relu_2l_res_s6"])
def test_table_layout_and_zero_padding(name):
    cs = TR.case(name)
    ds, DS, H = cs["ds"], cs["DS"], 32
    for k, (hidden, width) in enumerate(VALUES):
        val = value_for(cs, k, "tanh")
        m = model_of(cs)
        m.set_value(val["Ws"], val["bs"])
        tab = m.value["table"]
        assert tab.dtype == f32 and tab.shape == (VR.n_floats(DS),) == (H * DS + 1121,)
        same_bits("table", tab, VR.pack(val["Ws"], val["bs"], ds, DS))
        W1, b1, W2, b2, w3, b3 = VR.unpack(tab, DS)
        same_bits("W1", W1[:width, :ds], val["Ws"][0])
        assert not W1[width:].any() and not W1[:, ds:].any() and not b1[width:].any() and not w3[width:].any()
        same_bits("b3", b3, val["bs"][-1])
        if hidden == 2:
            same_bits("W2", W2[:width, :width], val["Ws"][1])
            assert not W2[width:].any() and not W2[:, width:].any() and not b2[width:].any()
            same_bits("w3", w3[:width], val["Ws"][2][0])
        else:
            assert not W2.any() and not b2.any()
            same_bits("w3", w3[:width], val["Ws"][1][0])
        assert m.value["hidden_layers"] == hidden and m.native_inputs()["mlp"]["value"]["version"] == m.value_version


def test_set_value_module():
    cs = TR.case("mlp41_relu_2l_res")
    m = model_of(cs)
    net = torch.nn.Sequential(torch.nn.Linear(4, 16), torch.nn.ReLU(), torch.nn.Linear(16, 8), torch.nn.ReLU(), torch.nn.Linear(8, 1))
    m.set_value_module(net, weight=2.0, replace_terminal=True)
    assert (m.value["hidden_layers"], m.value["activation"], m.value["weight"], m.value["replace_terminal"]) == (2, "relu", 2.0, True)
    s = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (50, 4)).astype(f32))
    assert torch.allclose(m.value_of(s), net(s)[:, 0].detach(), atol=1e-6)
    for bad in (torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Sigmoid(), torch.nn.Linear(8, 1)),
                torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.ReLU(), torch.nn.Linear(8, 1, bias=False)),
                torch.nn.Sequential(torch.nn.Linear(4, 1))):
        with pytest.raises(ValueError):
            m.set_value_module(bad)


# ------------------------------------------------------------------------------ what is refused
def test_every_value_error():
    cs = TR.case("mlp42_relu_1l_abs")
    m = model_of(cs)
    rng = np.random.default_rng(2)

    def net(dims):
        return ([rng.standard_normal((o, i)).astype(f32) for i, o in zip(dims[:-1], dims[1:])],
                [rng.standard_normal(o).astype(f32) for o in dims[1:]])

    with pytest.raises(ValueError, match="no value"):
        m.terminal_cost(torch.zeros(3, 4))
    for name, dims in (("two outputs", [4, 8, 2]), ("33 units", [4, 33, 1]), ("33 units in layer 2", [4, 8, 33, 1]),
                       ("three hidden layers", [4, 8, 8, 8, 1]), ("no hidden layer", [4, 1]), ("wrong input width", [5, 8, 1])):
        with pytest.raises(ValueError):
            m.set_value(*net(dims))
        assert m.value is None, name
    Ws, bs = net([4, 8, 1])
    for w in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="finite"):
            m.set_value(Ws, bs, weight=w)
    with pytest.raises(ValueError, match="activation"):
        m.set_value(Ws, bs, activation="sigmoid")
    Wn = [Ws[0].copy(), Ws[1]]
    Wn[0][1, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        m.set_value(Wn, bs)
    with pytest.raises(ValueError):
        m.set_value(Ws, bs[:1])
    for call in (lambda: m.update_value(Ws, bs), lambda: m.set_value_weight(1.0)):
        with pytest.raises(ValueError, match="no value"):
            call()
    m.set_value(Ws, bs)
    with pytest.raises(ValueError, match="number of layers"):
        m.update_value(*net([4, 8, 8, 1]))
    with pytest.raises(ValueError, match="finite"):
        m.set_value_weight(float("nan"))
    m.set_value(None)
    with pytest.raises(ValueError, match="no value"):
        m.terminal_cost(torch.zeros(3, 4))


# ------------------------------------------------------------------------------ copies and versions
def test_deepcopy_carries_the_value_and_the_versions_move():
    from envs import MLPEnsemble

    cs = TR.case("mlp41_relu_2l_res")
    m = model_of(cs)
    v0 = m.value_version
    val, val2 = value_for(cs, 1, "tanh"), value_for(cs, 5, "tanh")
    m.set_value(val["Ws"], val["bs"], weight=0.5, replace_terminal=True)
    v1 = m.value_version
    assert v1 > v0
    twin = copy.deepcopy(m)
    s = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (20, 4)).astype(f32))
    assert torch.equal(twin.terminal_cost(s), m.terminal_cost(s))
    assert twin.value is not m.value and twin.value["table"] is not m.value["table"]
    assert np.array_equal(twin.value["table"], m.value["table"]) and twin.value["weight"] == 0.5 and twin.value["replace_terminal"]
    m.update_value(val2["Ws"], val2["bs"])
    v2 = m.value_version
    assert v2 > v1 and not np.array_equal(twin.value["table"], m.value["table"])
    assert (m.value["weight"], m.value["replace_terminal"], m.value["activation"]) == (0.5, True, "tanh")
    assert not torch.equal(twin.terminal_cost(s), m.terminal_cost(s))  # (the copy keeps the old critic)
    m.set_value_weight(2.0)
    assert m.value_version > v2 and m.value["weight"] == 2.0 and twin.value["weight"] == 0.5
    v3 = m.value_version
    m.set_value(None)
    assert m.value_version > v3 and m.value is None and m.native_inputs()["mlp"]["value"] is None
    # an ensemble: one value, forwarded to every member; the tagged callable is the nominal member's
    ens = MLPEnsemble([model_of(cs), model_of(cs)])
    ens.set_value(val["Ws"], val["bs"], weight=0.25)
    assert all(np.array_equal(ens.member(e).value["table"], ens.member(0).value["table"]) for e in range(2))
    assert torch.equal(ens.terminal_cost(s), ens.member(0).terminal_cost(s)) and ens.value["weight"] == 0.25
    ens.set_value_weight(3.0)
    ens.update_value(val2["Ws"], val2["bs"])
    assert all(ens.member(e).value["weight"] == 3.0 for e in range(2))
    twin = copy.deepcopy(ens)
    assert torch.equal(twin.terminal_cost(s), ens.terminal_cost(s))
    from pi_mpc.native import resolve
    for owner in (m, ens):
        tag, who = resolve(owner.terminal_cost)
        assert (tag.model, tag.role, tag.per_owner) == ("mlp41", "terminal", True) and who is owner


# ------------------------------------------------------------------------------ the functor, compiled for the host
@pytest.fixture(scope="module")
def emul_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mlp_value_emul") / "libmlp_value_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, SRC])
    return C.CDLL(so)


def emul(lib, cs, fast, U, val, ref=None, angular=(), weight=1.0, replace=False):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    N, T, dc = U.shape
    ds, DS = cs["ds"], cs["DS"]
    table, params = np.ascontiguousarray(cs["table"], f32), np.ascontiguousarray(cs["params"], f32)
    x0, U = np.ascontiguousarray(cs["x0"], f32), np.ascontiguousarray(U, f32)
    ref = None if ref is None else np.ascontiguousarray(ref, f32)
    vt = None if val is None else VR.pack(val["Ws"], val["bs"], ds, DS)
    costs, V = np.full(N, np.nan, f32), np.full(N, np.nan, f32)
    lib.mlp_value_emul_rollout.argtypes = [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                           C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rc = lib.mlp_value_emul_rollout(DS, dc, int(fast), p(table), int(table.size), cs["hidden_layers"], int(cs["activation"] == "tanh"),
                                    int(cs["residual"]), p(params), int(params.size), p(ref), 0 if ref is None else len(ref),
                                    TR.mask(angular), p(vt), 0 if vt is None else int(vt.size),
                                    0 if val is None else val["hidden_layers"], int(val is not None and val["activation"] == "tanh"),
                                    float(weight), int(replace), p(x0), p(U), N, T, p(costs), p(V))
    assert rc == 0
    return costs, V


@pytest.mark.parametrize("name", RELU)
def test_host_functor_equals_the_restatement_bit_for_bit(emul_lib, name):
    cs = TR.case(name)
    for T in (1, cs["horizons"][-1]):
        U = TR.actions(cs, 5, 64, T)
        ref = TR.reference(cs, T)
        for k in range(len(VALUES)):
            val = value_for(cs, k, "relu")
            for replace in (False, True):
                for table, angular in ((None, ()), (ref, cs["angular"])):
                    want = VR.rollout(cs, val, U, ref=table, angular=angular, weight=-1.5, replace_terminal=replace)[0]
                    got, _ = emul(emul_lib, cs, 0, U, val, table, angular, -1.5, replace)
                    same_bits(f"{name} T{T} value {k} replace {replace} ref {table is not None}", got, want)
                    assert not np.array_equal(want, VR.rollout(cs, None, U, ref=table, angular=angular)[0])
        # weight 0 (not replacing) and no value at all: the bits of the tracking restatement
        plain = TR.rollout(cs, None, (), U)[0]
        same_bits(f"{name} T{T} weight 0", emul(emul_lib, cs, 0, U, value_for(cs, 0, "relu"), weight=0.0)[0], plain)
        same_bits(f"{name} T{T} no value", emul(emul_lib, cs, 0, U, None)[0], plain)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("name", TANH)
def test_host_functor_tanh_and_fast_math_within_the_band(emul_lib, name, fast):
    cs = TR.case(name)
    T = cs["horizons"][-1]
    U = TR.actions(cs, 6, 100, T)
    worst = 0.0
    for k in range(len(VALUES)):
        val = value_for(cs, k, "tanh")
        for replace in (False, True):
            c32, _, mag = VR.rollout(cs, val, U, weight=2.0, replace_terminal=replace)
            c64 = VR.rollout(cs, val, U, f64, weight=2.0, replace_terminal=replace)[0]
            limit, yard = VR.band(c32, c64, mag)
            got, _ = emul(emul_lib, cs, fast, U, val, weight=2.0, replace=replace)
            err = np.abs(got.astype(f64) - c64)
            worst = max(worst, float(err.max() / yard))
            assert np.all(np.isfinite(got)) and np.all(err <= limit), (name, k, replace, err.max())
    print(f"[mlp-value] host functor {name} math {fast}: ratio {worst:.2f} of the fp32 band")


def test_flags_word_and_the_choice_of_the_instantiation(emul_lib):
    lib = emul_lib
    for ds in (4, 8):
        assert lib.mlp_value_emul_floats(ds) == VR.n_floats(ds) == 32 * ds + 1121
    for arch in range(8):
        for ang in (0, 1, 0x81, 0xff):
            for v in range(8):
                w = lib.mlp_value_emul_flags_word(arch, ang, v) & 0xffffffff
                assert (w & 7, (w >> 8) & 0xff, (w >> 16) & 7, w >> 19) == (arch, ang, v, 0)
    # a value alone selects the instantiation that carries it; none of the three keeps the default one
    assert lib.mlp_value_emul_tracking(7, 0, 0) == 0 and lib.mlp_value_emul_tracking(7, 0, 1) == 1
    assert lib.mlp_value_emul_tracking(0, 2, 0) == 1


def test_standalone_program_passes_the_sanitizers(tmp_path):
    exe = str(tmp_path / "mlp_value_emul_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-DMLP_VALUE_EMUL_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "80 runs" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
