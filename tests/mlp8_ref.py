"""numpy restatement of the 8-state learned-dynamics models (MPPI_MODEL_MLP81 / MLP82 / MLP84; include/mppi_hip.h: mppi_set_mlp)
and the case table the host and the GPU tests share.  tests/mlp_ref.py restates the 4-state ids; what does not depend on the
state width (the activation, the band rule, the contraction scaling) is imported from there.

Two evaluations of the same network and cost, over a batch of action sequences U [N, T, dc] from one start x0 [8]:
  fp32   every operation rounded on its own, in the order the header fixes (numpy's element-wise float32 arithmetic; only the
         reduction indices are Python loops), the T stage costs and the terminal cost added in float64 and rounded once —
         what option "math" = 0 computes, bit for bit with relu;
  fp64   the same network in float64 throughout (weights, states and costs): the value both approximate.
"""
import numpy as np

from mlp_ref import _act, _spectral_scale, band  # noqa: F401  (width-independent; band is re-exported for the tests)
from mlp_ref import HORIZONS as HORIZONS4

f32, f64 = np.float32, np.float64
H, DS = 32, 8


def n_floats(dc):
    return H * (DS + dc) + H + H * H + H + DS * H + DS


def pack(Ws, bs, dc):
    """Layers as [out, in] matrices of a network with ds <= 8 states, input [s0..s(ds-1), u] -> the padded table: zero rows,
    columns and biases, the controls' columns behind EIGHT state columns."""
    ds = Ws[-1].shape[0]
    assert Ws[0].shape[1] == ds + dc and 1 <= ds <= DS
    IN = DS + dc
    W1, b1 = np.zeros((H, IN), f32), np.zeros(H, f32)
    W2, b2 = np.zeros((H, H), f32), np.zeros(H, f32)
    W3, b3 = np.zeros((DS, H), f32), np.zeros(DS, f32)
    W1[:Ws[0].shape[0], :ds] = Ws[0][:, :ds]
    W1[:Ws[0].shape[0], DS:] = Ws[0][:, ds:]
    b1[:len(bs[0])] = bs[0]
    if len(Ws) == 3:
        W2[:Ws[1].shape[0], :Ws[1].shape[1]] = Ws[1]
        b2[:len(bs[1])] = bs[1]
    W3[:ds, :Ws[-1].shape[1]] = Ws[-1]
    b3[:ds] = bs[-1]
    return np.concatenate([a.reshape(-1) for a in (W1, b1, W2, b2, W3, b3)]).astype(f32)


def unpack(table, dc):
    IN = DS + dc
    t = np.asarray(table, f32)
    assert t.shape == (n_floats(dc),)
    cut = np.cumsum([0, H * IN, H, H * H, H, DS * H, DS])
    parts = [t[a:b] for a, b in zip(cut[:-1], cut[1:])]
    return (parts[0].reshape(H, IN), parts[1], parts[2].reshape(H, H), parts[3], parts[4].reshape(DS, H), parts[5])


def step(layers, s, u, layers2, activation, residual):
    """s [N, ds], u [N, dc] -> next state; the dtype of `s` is the arithmetic.  The layers may be the table's padded ones
    (ds = 8) or narrower (W1 [h, ds + dc], W2 [h, h], W3 [ds, h])."""
    W1, b1, W2, b2, W3, b3 = layers
    x = np.concatenate([s, u], axis=1)
    z = np.broadcast_to(b1, (len(s), len(b1))).copy()
    for i in range(x.shape[1]):
        z = z + W1[:, i] * x[:, i:i + 1]
    h = _act(z, activation)
    if layers2 == 2:
        z = np.broadcast_to(b2, (len(s), len(b2))).copy()
        for i in range(W2.shape[1]):
            z = z + W2[:, i] * h[:, i:i + 1]
        h = _act(z, activation)
    o = np.broadcast_to(b3, (len(s), len(b3))).copy()
    for j in range(W3.shape[1]):
        o = o + W3[:, j] * h[:, j:j + 1]
    return s + o if residual else o


def cost(params, s, u):
    """params = g[8], q[8], r[dc]; s [N, ds <= 8] -> (c [N], sum of |terms| [N]) in the dtype of `s`."""
    dc = u.shape[1]
    g, q, r = params[0:DS], params[DS:2 * DS], params[2 * DS:2 * DS + dc]
    c = np.zeros(len(s), s.dtype)
    mag = np.zeros(len(s), f64)
    for m in range(s.shape[1]):
        d = s[:, m] - g[m]
        term = q[m] * (d * d)
        c = c + term
        mag += np.abs(term)
    for k in range(dc):
        term = r[k] * (u[:, k] * u[:, k])
        c = c + term
        mag += np.abs(term)
    return c, mag


def rollout(table, params, hidden_layers, activation, residual, x0, U, dtype=f32, layers=None):
    """-> (costs [N] (float32 for dtype=f32: the float64 sum of the fp32 stage costs rounded once; else float64),
    states [N, T + 1, ds], sum of |cost terms| [N] (float64)).  `layers`: evaluate these (unpadded) layers from a start of THEIR
    state width instead of the table (ds = 8)."""
    U = np.asarray(U)
    N, T, dc = U.shape
    layers = tuple(np.asarray(a, f32).astype(dtype) for a in (unpack(table, dc) if layers is None else layers))
    ds = layers[4].shape[0]
    P = np.asarray(params, f32).astype(dtype)
    s = np.broadcast_to(np.asarray(x0, f32)[:ds].astype(dtype), (N, ds)).copy()
    S = np.empty((N, T + 1, ds), dtype)
    acc, mag = np.zeros(N, f64), np.zeros(N, f64)
    Ud = U.astype(dtype)
    for t in range(T):
        S[:, t] = s
        c, m = cost(P, s, Ud[:, t])
        acc += c.astype(f64)
        mag += m
        s = step(layers, s, Ud[:, t], hidden_layers, activation, residual)
    S[:, T] = s
    c, m = cost(P, s, np.zeros((N, dc), dtype))
    acc += c.astype(f64)
    mag += m
    return (acc.astype(f32) if dtype == f32 else acc), S, mag


# ---------------------------------------------------------------------------------------------- the case table
def make_net(seed, dc, hidden, activation, residual, width=H, ds=DS, out_scale=None):
    """mlp_ref.make_net for `ds` states: every weight matrix scaled to a spectral norm of at most 0.9, `residual` only with
    the output layer scaled by 0.05, so that rounding does not grow along the horizon."""
    rng = np.random.default_rng(8000 + seed)
    dims = [ds + dc] + [width] * hidden + [ds]
    Ws = [_spectral_scale(rng.standard_normal((o, i)), 0.9) for i, o in zip(dims[:-1], dims[1:])]
    bs = [(0.1 * rng.standard_normal(o)).astype(f32) for o in dims[1:]]
    if residual:
        s = 0.05 if out_scale is None else out_scale
        Ws[-1] = (Ws[-1] * f32(s)).astype(f32)
        bs[-1] = (bs[-1] * f32(s)).astype(f32)
    return Ws, bs


def make_params(seed, dc, ds=DS):
    """g[8], q[8], r[dc]; the entries of g and q beyond a narrower state are zero (what MLPModel8 hands the device)."""
    rng = np.random.default_rng(9000 + seed)
    g, q = np.zeros(DS), np.zeros(DS)
    g[:ds] = rng.uniform(-0.5, 0.5, ds)
    q[:ds] = rng.uniform(0.5, 2.0, ds)
    r = rng.uniform(0.01, 0.1, dc)
    return np.concatenate([g, q, r]).astype(f32)


LIMITS = {1: dict(u_min=[-1.5], u_max=[1.5], sigmas=[0.8]), 2: dict(u_min=[-1.0, -2.0], u_max=[1.5, 2.0], sigmas=[0.6, 1.0]),
          4: dict(u_min=[-1.0, -2.0, -0.5, -1.5], u_max=[1.5, 2.0, 0.75, 1.0], sigmas=[0.6, 1.0, 0.4, 0.7])}
X0 = f32([0.3, -0.2, 0.5, 0.1, -0.4, 0.25, 0.15, -0.1])

# (name, dc, hidden layers, activation, residual, width, states of the network): the three ids x one and two layers x residual
# on and off x both activations, a 20-wide network (against its padded form) and one 6-state network per control width
# (the padding: components 6 and 7 stay zero)
CASES = [(f"mlp8{dc}_{act}_{hl}l_{'res' if res else 'abs'}", dc, hl, act, res, H, DS)
         for dc in (1, 2, 4) for act in ("relu", "tanh") for hl in (1, 2) for res in (False, True)]
CASES += [("mlp84_relu_2l_res_w20", 4, 2, "relu", True, 20, DS)]
CASES += [("mlp81_relu_2l_res_s6", 1, 2, "relu", True, H, 6), ("mlp82_tanh_2l_res_s6", 2, 2, "tanh", True, H, 6),
          ("mlp84_relu_1l_abs_s6", 4, 1, "relu", False, H, 6)]
# horizons that reach every copy of the rollout loop (steps per float4 group: 4 / dc; dc = 4: one step per group, so both
# parities of the drain halves, a horizon of one group and one past two groups of four), sample counts: one tile, a ragged
# tile, 65 tiles
HORIZONS = {1: HORIZONS4[1], 2: HORIZONS4[2], 4: (1, 2, 3, 4, 5, 9)}
SAMPLES = (64, 100, 4160)


def case(name):
    for i, c in enumerate(CASES):
        if c[0] == name:
            _, dc, hl, act, res, width, ds = c
            Ws, bs = make_net(i, dc, hl, act, res, width, ds)
            x0 = X0.copy()
            x0[ds:] = 0
            return dict(name=name, model=f"mlp8{dc}", dc=dc, ds=ds, hidden_layers=hl, activation=act, residual=res, width=width,
                        Ws=Ws, bs=bs, table=pack(Ws, bs, dc), params=make_params(i, dc, ds), x0=x0, **LIMITS[dc])
    raise KeyError(name)


def actions(seed, N, T, dc):
    """Clamped random actions like the solver's (bounds of LIMITS)."""
    rng = np.random.default_rng(seed)
    lim = LIMITS[dc]
    U = rng.standard_normal((N, T, dc)) * np.asarray(lim["sigmas"])
    return np.clip(U, lim["u_min"], lim["u_max"]).astype(f32)
