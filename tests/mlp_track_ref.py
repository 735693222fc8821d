"""numpy restatement of the learned-dynamics models' TRACKING cost (include/mppi_hip.h: mppi_set_mlp_reference,
mppi_set_mlp_angular) and the inputs the host and the GPU tests share.  Networks, limits, HORIZONS and SAMPLES are those of
tests/mlp_ref.py (4 states) and tests/mlp8_ref.py (8 states); this file adds the per-step goals, the angular components and the
wrapped error:

    row(t) = g_t[DS] then q_t[DS]                       (no reference: g_t = g, q_t = q of the parameters)
    d[m]   = s[m] - g_t[m];   m angular:  k = rint(d[m] * INV_TWO_PI);  d[m] = d[m] - TWO_PI * k
    c      = sum_m ascending c + q_t[m] * (d[m] * d[m]);  then sum_k ascending c + r[k] * (u[k] * u[k])
    the stage cost of step t reads row t, the terminal cost row T - 1 with u = 0

fp32: every operation rounded on its own (numpy's element-wise float32 arithmetic, np.rint = round half to even); fp64: the
same in float64 with the same two constants (they ARE the float32 values).
"""
import numpy as np

import mlp8_ref as R8
import mlp_ref as R4

f32, f64 = np.float32, np.float64
TWO_PI, INV_TWO_PI = f32(6.2831855), f32(0.15915494)
band = R4.band

# One two-layer and one one-layer network per id, relu (bit for bit) and tanh (the band), out of the two case tables, and the
# two 6-state networks (the last REAL component is 5: the padded components are never angular).
_BASE = [f"mlp4{dc}_{act}_{hl}" for dc in (1, 2) for act in ("relu", "tanh") for hl in ("2l_res", "1l_abs")]
_BASE += [f"mlp8{dc}_{act}_{hl}" for dc in (1, 2, 4) for act in ("relu", "tanh") for hl in ("2l_res", "1l_abs")]
_BASE += ["mlp81_relu_2l_res_s6", "mlp82_tanh_2l_res_s6"]
CASES = list(_BASE)
RELU = [n for n in CASES if "_relu_" in n]
TANH = [n for n in CASES if "_tanh_" in n]
SAMPLES = R4.SAMPLES
assert SAMPLES == R8.SAMPLES


def module_of(name):
    return R4 if name.startswith("mlp4") else R8


def case(name):
    """The case of mlp_ref / mlp8_ref under one set of keys, plus `angular`: the first and the last real state component."""
    R = module_of(name)
    cs = dict(R.case(name))
    cs.setdefault("model", name[:5])
    cs.setdefault("ds", R.DS)
    cs.setdefault("x0", R.X0.copy())
    cs["DS"] = R.DS
    cs["angular"] = (0, cs["ds"] - 1)
    cs["horizons"] = R.HORIZONS[cs["dc"]]
    return cs


def mask(angular):
    return sum(1 << m for m in angular)


def reference(cs, T, seed=0, extra=0, finite_extra=0):
    """The padded table [T + finite_extra + extra, 2 * DS]: g_t and q_t differ in every row, q_t in [0.5, 2]; the goals of the
    angular components are drawn from +-[3, 9] (the first two rows from +-[4, 9]) with the sign alternating from row to row (the
    cases' states stay near +-0.5: a goal near 0 would never wrap), the others from [-0.5, 0.5].  `finite_extra` more finite rows follow (what an off-by-one
    would read), then `extra` rows of NaN (what nobody may read)."""
    ds, DS = cs["ds"], cs["DS"]
    rng = np.random.default_rng([seed, T, len(cs["name"]), sum(map(ord, cs["name"]))])
    pool = T + 8  # (always drawn in full, so the first T rows do not depend on how many follow)
    assert finite_extra <= 8
    full = np.zeros((pool, 2 * DS), f32)
    full[:, :ds] = rng.uniform(-0.5, 0.5, (pool, ds))
    for j, m in enumerate(cs["angular"]):
        sign = np.where((np.arange(pool) + j) % 2 == 0, 1.0, -1.0)
        mag = rng.uniform(3.0, 9.0, pool)
        mag[:2] = 4.0 + (mag[:2] - 3.0) * (5.0 / 6.0)  # (rows 0 and 1 from [4, 9]: a two-row table wraps with both signs)
        full[:, m] = sign * mag
    full[:, DS:DS + ds] = rng.uniform(0.5, 2.0, (pool, ds))
    rows = T + finite_extra
    return np.concatenate([full[:rows], np.full((extra, 2 * DS), np.nan, f32)])


def constant_reference(cs, T):
    """goal, q of the parameters in every row: with no angular component the tracking cost IS the plain cost."""
    DS = cs["DS"]
    return np.tile(np.asarray(cs["params"][:2 * DS], f32), (T, 1))


def wrap(d):
    """-> (wrapped d, k, d * INV_TWO_PI) in the dtype of d."""
    ty = d.dtype.type
    turns = d * ty(INV_TWO_PI)
    k = np.rint(turns)
    return d - ty(TWO_PI) * k, k, turns


def cost(row, r, angular, s, u, stats=None):
    """row = g[DS] then q[DS] -> (c [N], sum of |terms| [N]) in the dtype of `s` (s [N, ds <= DS])."""
    DS = len(row) // 2
    c = np.zeros(len(s), s.dtype)
    mag = np.zeros(len(s), f64)
    for m in range(s.shape[1]):
        d = s[:, m] - row[m]
        if m in angular:
            d, k, turns = wrap(d)
            if stats is not None:
                stats.setdefault(m, []).append((k.astype(f64), np.abs(turns.astype(f64) - k.astype(f64))))
        term = row[DS + m] * (d * d)
        c = c + term
        mag += np.abs(term)
    for j in range(u.shape[1]):
        term = r[j] * (u[:, j] * u[:, j])
        c = c + term
        mag += np.abs(term)
    return c, mag


def rollout(cs, ref, angular, U, dtype=f32, x0=None, shift=0, terminal_row=None, stats=None, table=None):
    """-> (costs [N], states [N, T + 1, ds], sum of |cost terms| [N]), as mlp_ref.rollout returns them.  ref: the table
    [rows >= T, 2 * DS] or None (goal and q of the parameters).  `shift` and `terminal_row` restate the two off-by-one mistakes
    (stage t reading row t + shift; the terminal cost reading another row than T - 1).  `table`: another member's weights."""
    R = module_of(cs["name"])
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
        c, m = cost(rows[t + shift], r, angular, s, Ud[:, t], stats)
        acc += c.astype(f64)
        mag += m
        s = R.step(layers, s, Ud[:, t], cs["hidden_layers"], cs["activation"], cs["residual"])
    S[:, T] = s
    c, m = cost(rows[T - 1 if terminal_row is None else terminal_row], r, angular, s, np.zeros((N, dc), dtype), stats)
    acc += c.astype(f64)
    mag += m
    return (acc.astype(f32) if dtype == f32 else acc), S[:, :, :ds], mag


def actions(cs, seed, N, T):
    return module_of(cs["name"]).actions(seed, N, T, cs["dc"])
