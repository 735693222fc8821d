"""The cases the host and the GPU tests of the model ensembles share (envs.MLPEnsemble; include/mppi_hip.h:
mppi_set_mlp_ensemble, mppi_set_particle_members): seeded random networks, every member a draw of its own.

Weights and biases are 0.3 x standard normal (the states of every case stay finite over the horizons used); the tables are
tests/mlp_ref.py's packing, so a member's table is what MLPModel builds from the same layers.  Four architectures reach both
models, one and two hidden layers, both activations and the residual switch on and off.
"""
import numpy as np

import mlp_ref as R

f32 = np.float32
SCALE = 0.3
# name -> (dc, hidden layers, activation, residual)
ARCHS = {"mlp41_relu_2l_res": (1, 2, "relu", True), "mlp42_tanh_1l_abs": (2, 1, "tanh", False),
         "mlp41_tanh_1l_res": (1, 1, "tanh", True), "mlp42_relu_2l_abs": (2, 2, "relu", False)}
SIZES_N = (65, 300)  # five tiles with a partial last one (a block with one live wave); two tiles
HORIZONS = (7, 8)    # both parities of the two-steps-per-group loop for dc = 2
E, P = 3, 5
MEMBERS = (2, 0, 1, 2, 0)
PARTS = (R.X0[None, :] + f32([[0.0, 0.0, 0.0, 0.0], [0.1, -0.05, 0.02, 0.03], [-0.2, 0.1, 0.05, -0.1], [0.05, 0.2, -0.1, 0.0],
                              [-0.1, -0.1, 0.1, 0.1]])).astype(f32)


def net(seed, dc, hidden_layers, width=R.H):
    rng = np.random.default_rng(seed)
    dims = [R.DS + dc] + [width] * hidden_layers + [R.DS]
    Ws = [(SCALE * rng.standard_normal((o, i))).astype(f32) for i, o in zip(dims[:-1], dims[1:])]
    bs = [(SCALE * rng.standard_normal(o)).astype(f32) for o in dims[1:]]
    return Ws, bs


def case(name, n_members=E, seed=0):
    """-> dict: the architecture, the cost parameters and limits of tests/mlp_ref.py, and per member (Ws, bs) and its table."""
    dc, hl, act, res = ARCHS[name]
    base = 1000 * (1 + sorted(ARCHS).index(name)) + 100 * seed
    nets = [net(base + e, dc, hl) for e in range(n_members)]
    return dict(name=name, model=f"mlp4{dc}", dc=dc, hidden_layers=hl, activation=act, residual=res, nets=nets,
                tables=np.stack([R.pack(Ws, bs, dc) for Ws, bs in nets]), params=R.make_params(3, dc), **R.LIMITS[dc])


def models(cs):
    """One envs.MLPModel per member."""
    from envs import MLPModel

    p = cs["params"]
    return [MLPModel(Ws, bs, activation=cs["activation"], residual=cs["residual"], goal=p[:4], q=p[4:8], r=p[8:])
            for Ws, bs in cs["nets"]]


def ref(cs, e, x0, U, dtype=f32, table=None):
    """tests/mlp_ref.py's rollout through member e's table from x0."""
    return R.rollout(cs["tables"][e] if table is None else table, cs["params"], cs["hidden_layers"], cs["activation"],
                     cs["residual"], x0, U, dtype)
