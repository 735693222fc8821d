"""numpy restatement of the learned-dynamics models' TERMINAL VALUE (include/mppi_hip.h: mppi_set_mlp_value) and the value
networks the host and the GPU tests share: tests/mlp_track_ref.py's rollout with the value at the end.

    z1[j] = b1[j]; for i ascending: z1[j] = z1[j] + W1[j][i] * s[i];   h1 = act(z1)
    z2[j] = b2[j]; for i ascending: z2[j] = z2[j] + W2[j][i] * h1[i];  h2 = act(z2)          (two hidden layers)
    V = b3; for j ascending: V = V + w3[j] * h          (h = h2, or h1 with one hidden layer)
    terminal = quad_T + (weight * V),   or weight * V alone with replace_terminal

fp32: every operation rounded on its own; fp64: the same in float64.  The magnitude sum |terms| carries the value's terms
(|weight * V| and, inside V, |b3| and every |w3[j] * h[j]|), so that mlp_ref.band applies unchanged.
"""
import numpy as np

import mlp_track_ref as TR

f32, f64 = np.float32, np.float64
H = 32
band = TR.band


def n_floats(DS):
    return H * DS + H + H * H + H + H + 1


def pack(Ws, bs, ds, DS):
    """Layers as torch.nn.Linear lays them out (W1 [h1, ds], (W2 [h2, h1],) W3 [1, h]) -> the padded table."""
    W1, b1 = np.zeros((H, DS), f32), np.zeros(H, f32)
    W2, b2 = np.zeros((H, H), f32), np.zeros(H, f32)
    w3, b3 = np.zeros(H, f32), np.zeros(1, f32)
    W1[:Ws[0].shape[0], :ds] = Ws[0]
    b1[:len(bs[0])] = bs[0]
    if len(Ws) == 3:
        W2[:Ws[1].shape[0], :Ws[1].shape[1]] = Ws[1]
        b2[:len(bs[1])] = bs[1]
    w3[:Ws[-1].shape[1]] = Ws[-1][0]
    b3[:] = bs[-1]
    return np.concatenate([a.reshape(-1) for a in (W1, b1, W2, b2, w3, b3)]).astype(f32)


def unpack(table, DS):
    t = np.asarray(table, f32)
    assert t.shape == (n_floats(DS),)
    cut = np.cumsum([0, H * DS, H, H * H, H, H, 1])
    p = [t[a:b] for a, b in zip(cut[:-1], cut[1:])]
    return p[0].reshape(H, DS), p[1], p[2].reshape(H, H), p[3], p[4], p[5]


def make_value(seed, ds, hidden, activation, width=H, scale=1.0):
    """A random value network over `ds` state components: hidden layers of `width` units.  The first layer is wide enough in
    weight (|W1| ~ 1) and bias that hidden units of BOTH signs occur on the cases' states (checked by the host test)."""
    rng = np.random.default_rng(7000 + seed)
    dims = [ds] + [width] * hidden + [1]
    Ws = [(rng.standard_normal((o, i)) / np.sqrt(max(i, 4) / 4.0)).astype(f32) for i, o in zip(dims[:-1], dims[1:])]
    bs = [(0.3 * rng.standard_normal(o)).astype(f32) for o in dims[1:]]
    Ws[-1] = (Ws[-1] * f32(scale)).astype(f32)
    return dict(Ws=Ws, bs=bs, hidden_layers=hidden, activation=activation, width=width)


def _act(z, activation):
    return np.tanh(z) if activation == "tanh" else np.maximum(z, z.dtype.type(0))


def value(layers, s, hidden_layers, activation, want_hidden=False):
    """s [N, DS] (zero-padded) -> (V [N], sum of |terms of V| [N]); the dtype of `s` is the arithmetic."""
    W1, b1, W2, b2, w3, b3 = layers
    n = len(s)
    z = np.broadcast_to(b1, (n, H)).copy()
    for i in range(s.shape[1]):
        z = z + W1[:, i] * s[:, i:i + 1]
    z1 = z
    h = _act(z, activation)
    if hidden_layers == 2:
        z = np.broadcast_to(b2, (n, H)).copy()
        for i in range(H):
            z = z + W2[:, i] * h[:, i:i + 1]
        h = _act(z, activation)
    v = np.broadcast_to(b3, (n,)).copy()
    mag = np.full(n, abs(float(b3[0])), f64)
    for j in range(H):
        term = w3[j] * h[:, j]
        v = v + term
        mag += np.abs(term)
    return (v, mag, z1) if want_hidden else (v, mag)


def rollout(cs, val, U, dtype=f32, ref=None, angular=(), weight=1.0, replace_terminal=False, x0=None, table=None):
    """mlp_track_ref.rollout with the value behind the terminal cost.  val: make_value's dict (or {"table", "hidden_layers",
    "activation"}), None: no value.  -> (costs [N], states [N, T + 1, ds], sum of |cost terms| [N])."""
    R = TR.module_of(cs["name"])
    U = np.asarray(U)
    N, T, dc = U.shape
    DS, ds = cs["DS"], cs["ds"]
    layers = tuple(np.asarray(a, f32).astype(dtype) for a in R.unpack(cs["table"] if table is None else table, dc))
    P = np.asarray(cs["params"], f32).astype(dtype)
    r = P[2 * DS:2 * DS + dc]
    rows = (np.tile(P[:2 * DS], (T + 1, 1)) if ref is None else np.asarray(ref, f32).astype(dtype))
    x = np.asarray(cs["x0"] if x0 is None else x0, f32).astype(dtype)
    s = np.broadcast_to(x, (N, DS)).copy()
    S = np.empty((N, T + 1, DS), dtype)
    acc, mag = np.zeros(N, f64), np.zeros(N, f64)
    Ud = U.astype(dtype)
    for t in range(T):
        S[:, t] = s
        c, m = TR.cost(rows[t], r, angular, s, Ud[:, t])
        acc += c.astype(f64)
        mag += m
        s = R.step(layers, s, Ud[:, t], cs["hidden_layers"], cs["activation"], cs["residual"])
    S[:, T] = s
    c, m = TR.cost(rows[T - 1], r, angular, s, np.zeros((N, dc), dtype))
    if val is not None:
        vt = val["table"] if "table" in val else pack(val["Ws"], val["bs"], ds, DS)
        vl = tuple(np.asarray(a, f32).astype(dtype) for a in unpack(vt, DS))
        v, vmag = value(vl, s, val["hidden_layers"], val["activation"])
        w = dtype(f32(weight))
        wv = w * v
        if replace_terminal:
            c, m = wv, np.zeros(N, f64)
        else:
            c = c + wv
        m = m + np.abs(wv.astype(f64)) + abs(float(w)) * vmag
    acc += c.astype(f64)
    mag += m
    return (acc.astype(f32) if dtype == f32 else acc), S[:, :, :ds], mag
