"""Injected-cost cases for weights_reduce_kernel and weighted_variance_kernel: the launch geometry restated, the tables of
sample counts and row shapes, cost vectors that place live tiles on purpose, and the float64 reference of the sums.

Nothing here touches the GPU or the library.  tests/test_reduce_cases_host.py asserts that the tables reach what they claim;
tests/test_gpu_reduce_geometry.py runs them.
"""
from __future__ import annotations

import numpy as np

from test_gpu_covariance import weights64  # the fp32 weight argument of the kernels, everything after it float64

f32 = np.float32
WAVE = 64            # samples per tile
NW = 4               # waves per block (BLOCK / WAVE)
TPW = 8              # tiles per wave and round
GPW = 8              # float4 groups per wave and column chunk
CHG = NW * GPW       # float4 groups per column chunk
REDUCE_MAX_BLOCKS = 2048
DEFAULT_REDUCE_BLOCKS = 512
FOLD_IN_FINALIZE_MAX_ROWS = 64

LIVE_COST = 8.0
DEAD_GAP = 1.0e4     # fl32(-(8 + 1e4) + 8) = -1e4 and expf(-1e4) is exactly 0
MAX_LIVE = 2048


# ------------------------------------------------------------------------------ launch geometry
def ntiles(N):
    return (int(N) + WAVE - 1) // WAVE


def blocks(N, reduce_blocks=DEFAULT_REDUCE_BLOCKS):
    """Grid of the reduction (capi_solve.hip, mppi_weights_reduce: `blocks = min(reduce_blocks, (tiles + 3) / 4)`, then
    `max(1, min(blocks, REDUCE_MAX_BLOCKS))`)."""
    if reduce_blocks is None:
        reduce_blocks = DEFAULT_REDUCE_BLOCKS
    return max(1, min(int(reduce_blocks), (ntiles(N) + NW - 1) // NW, REDUCE_MAX_BLOCKS))


def coords(tile, B):
    """(round, q, block, wave) of a tile (mppi_reduce.hpp: `for (base0 = blockIdx.x * NW; base0 < tiles; base0 += nwaves * TPW)`
    with nwaves = B * NW, and phase A's `base0 + wid + q * nwaves`): tile = round * 32B + q * 4B + 4 * block + wave.
    Works on integers and integer arrays."""
    tile = np.asarray(tile, np.int64)
    rnd, r = np.divmod(tile, NW * TPW * B)
    q, r = np.divmod(r, NW * B)
    block, wave = np.divmod(r, NW)
    if tile.ndim == 0:
        return int(rnd), int(q), int(block), int(wave)
    return rnd, q, block, wave


def tile_of(rnd, q, block, wave, B):
    return ((rnd * TPW + q) * B + block) * NW + wave


# ------------------------------------------------------------------------------ row shape
def row_shape(T, dc):
    """(R, nchunks, [(full, rem) per chunk], ragged): R = ceil(T * dc / 4) float4 groups in chunks of 32 (capi_handle.hip,
    mppi_create: `nchunks = (R + chg - 1) / chg`); inside a chunk of ng groups every wave owns full = ng / 4 of them and
    rem = ng % 4 are left over (mppi_reduce.hpp: `ng = min(CHG, d.R - r0)`)."""
    row = T * dc
    R = (row + 3) // 4
    nchunks = (R + CHG - 1) // CHG
    per = []
    for c in range(nchunks):
        ng = min(CHG, R - c * CHG)
        per.append((ng // NW, ng % NW))
    return R, nchunks, per, row % 4 != 0


# ------------------------------------------------------------------------------ the tables
# (name, N, reduce_blocks option or None for the default)
SAMPLE_AXIS = [
    ("G1", 2048, 1),                 # one block, exactly one round
    ("G2", 2049, 1),                 # ... a second round of one lane
    ("G3", 5000, 1),                 # ... three rounds, the last one ragged
    ("G4", 4423, 2),                 # two blocks, two rounds (70 tiles of 64 per round)
    ("G4b", 8423, 2),                # two blocks, three rounds
    ("G5", 613, None),               # three blocks, the last with two waves
    ("G6_1", 1, None), ("G6_64", 64, None), ("G6_65", 65, None), ("G6_100", 100, None),
    ("G7", 131072 + 193, None),      # 512 blocks with q = 1 in use
    ("G8", 2 ** 20 + 65, None),      # the default grid's second round
    ("G9", 524288 + 100, 2048),      # 2048 blocks, the cap
]
EXPLORE_SPLIT = "G4"                 # this geometry runs with sample_offset = 3N, inherit_count = 3N + 3N/4
LARGEST = ("G8", "G9")               # T = 4 only
SAMPLE_AXIS_ROWS = [(4, 1), (87, 1), (50, 2)]  # (T, dc)
VARIANCE_GEOMETRIES = ("G1", "G2", "G3", "G4", "G4b", "G5", "G7", "G8")
VARIANCE_ROWS = [(4, 1), (50, 2)]
FOLD_GEOMETRY = "G7"
FOLD_LIVE_ROWS = (1, 63, 64, 65, 512)
ROW_TABLE_N = 613
CHAINS2_BY_RULE = (132, 1, 76800)    # (T, dc, N): 300 blocks x 2 chunks > 2 x 256 compute units


def geometry(name):
    for g in SAMPLE_AXIS:
        if g[0] == name:
            return g
    raise KeyError(name)


def sample_axis_rows(name):
    return SAMPLE_AXIS_ROWS[:1] if name in LARGEST else SAMPLE_AXIS_ROWS


def row_table():
    """[(R, T, dc, wide)]"""
    out = []
    for R in list(range(1, 35)) + [40, 63, 64, 65]:
        out += [(R, 4 * R, 1, False), (R, 4 * R - 1, 1, False)]
    for R in (1, 5, 13, 20, 23, 25, 28, 31, 33):
        out.append((R, 2 * R - 1, 2, False))  # T odd: the last group is half used
    for T, dc in ((27, 3), (43, 3), (21, 6)):
        out.append(((T * dc + 3) // 4, T, dc, True))
    return out


# ------------------------------------------------------------------------------ cost vectors
def _lane_in(tile, N, rng):
    return int(rng.integers(0, min(WAVE, N - tile * WAVE)))


def _costs_from_live(N, live):
    live = np.unique(np.asarray(live, np.int64))
    assert 1 <= len(live) <= MAX_LIVE and live[0] >= 0 and live[-1] < N
    costs = np.full(N, LIVE_COST + DEAD_GAP, f32)
    costs[live] = LIVE_COST
    return costs, live


def sparse_costs(N, B, rng, one_per_block=None):
    """(costs, live sample indices).  Live samples cost 8, all others 8 + 1e4: at lambda = 1 the weights are exactly 1 and 0.
    Default placement: sample 0, sample N - 1, lanes 0 and 63 of one tile, the first and last tile of every round, for every
    q a tile in the first and in the last block that has one, one tile per wave.
    one_per_block = (L, mode): one live sample in each of L blocks, mode "first" / "last" / "spread" (blocks floor(i * B / L));
    the sample sits in the block's LAST round, so a block with tiles in round 1 has none live in round 0."""
    tiles = ntiles(N)
    rnd, q, blk, wav = coords(np.arange(tiles), B)
    if one_per_block is not None:
        L, mode = one_per_block
        assert 1 <= L <= B
        chosen = {"first": np.arange(L), "last": np.arange(B - L, B), "spread": (np.arange(L) * B) // L}[mode]
        live = []
        for b in chosen:
            mine = np.nonzero(blk == b)[0]
            late = mine[rnd[mine] == rnd[mine].max()]
            t = int(rng.choice(late))
            live.append(t * WAVE + _lane_in(t, N, rng))
        return _costs_from_live(N, live)
    live = [0, N - 1]
    full_tiles = N // WAVE
    if full_tiles:
        t = int(rng.integers(0, full_tiles))
        live += [t * WAVE, t * WAVE + 63]
    picked = []
    for r in np.unique(rnd):
        mine = np.nonzero(rnd == r)[0]
        picked += [mine[0], mine[-1]]
    for qq in np.unique(q):
        mine = np.nonzero(q == qq)[0]
        picked.append(rng.choice(mine[blk[mine] == blk[mine].min()]))
        picked.append(rng.choice(mine[blk[mine] == blk[mine].max()]))
    for w in np.unique(wav):
        picked.append(rng.choice(np.nonzero(wav == w)[0]))
    for t in picked:
        live.append(int(t) * WAVE + _lane_in(int(t), N, rng))
    return _costs_from_live(N, live)


DENSE_KINDS = ("uniform", "equal", "offset", "inf")


def dense_costs(N, kind, rng):
    """(costs, lambda).
    uniform: spread a = 5.97 at lambda = 1: ESS / N = (2 / a) tanh(a / 2) = 1 / 3 for costs uniform on [0, a];
    equal: every weight 1; offset: a common 1e6 (cost spacing 1 / 16) with unit spread; inf: uniform with 20 % +inf."""
    if kind == "uniform":
        return (10.0 + 5.97 * rng.random(N)).astype(f32), 1.0
    if kind == "equal":
        return np.full(N, 3.5, f32), 0.7
    if kind == "offset":
        return (1.0e6 + rng.random(N)).astype(f32), 1.0
    if kind == "inf":
        c = (2.0 + 5.97 * rng.random(N)).astype(f32)
        dead = rng.random(N) < 0.2
        dead[int(rng.integers(0, N))] = False
        c[dead] = np.inf
        return c, 1.0
    raise KeyError(kind)


def one_per_block_plans(B):
    """The (L, mode) pairs a geometry of B blocks runs."""
    plans = [(1, "last"), (min(65, B), "spread"), (B, "first")]
    if B >= 64:
        plans += [(63, "first"), (64, "last")]
    out = []
    for p in plans:
        if p[0] >= 1 and p[0] not in [o[0] for o in out]:
            out.append(p)
    return out


def _seed(N, salt):
    return np.random.default_rng([int(N), int(salt)])


def sample_axis_costs(name, dense=("uniform", "inf")):
    """[(label, costs, lambda, live indices or None)] of one geometry: the sparse placement, its one-per-block plans and the
    dense kinds."""
    _, N, rb = geometry(name)
    B = blocks(N, rb)
    out = []
    c, live = sparse_costs(N, B, _seed(N, 1))
    out.append(("sparse", c, 1.0, live))
    for k, (L, mode) in enumerate(one_per_block_plans(B)):  # (B <= ceil(tiles / 4): every block owns a tile)
        c, live = sparse_costs(N, B, _seed(N, 10 + k), one_per_block=(L, mode))
        out.append((f"one_per_block_{L}_{mode}", c, 1.0, live))
    for k, kind in enumerate(dense):
        c, lam = dense_costs(N, kind, _seed(N, 100 + k))
        out.append((kind, c, lam, None))
    return out


def fold_costs():
    """[(label, costs, live)] on the fold geometry: L published rows, in the first, the last and evenly spread blocks."""
    _, N, rb = geometry(FOLD_GEOMETRY)
    B = blocks(N, rb)
    out = []
    for L in FOLD_LIVE_ROWS:
        for k, mode in enumerate(("first", "last", "spread")):
            if L == B and k:
                continue
            c, live = sparse_costs(N, B, _seed(N, 1000 + 3 * L + k), one_per_block=(L, mode))
            out.append((f"L{L}_{mode}", c, live))
    return out


def row_table_costs(i, N=ROW_TABLE_N):
    """Case i of the row table: [(label, costs, lambda, live or None)], one sparse and one dense vector (kinds in turn)."""
    B = blocks(N)
    c, live = sparse_costs(N, B, _seed(N, 2000 + i))
    kind = DENSE_KINDS[i % len(DENSE_KINDS)]
    d, lam = dense_costs(N, kind, _seed(N, 3000 + i))
    return [("sparse", c, 1.0, live), (kind, d, lam, None)]


# ------------------------------------------------------------------------------ the reference
def reference(U, costs, lam):
    """(sum e, sum e^2, sum e*c, A[T*dc]) in float64 from the weights of weights64; terms with e = 0 are left out (their cost may
    be +inf).  A = sum_i e_i U_i is the un-normalised row."""
    e, _ = weights64(costs, lam)
    live = np.nonzero(e != 0.0)[0]
    e = e[live]
    c = np.asarray(costs, f32)[live].astype(np.float64)
    U = np.asarray(U)
    A = np.zeros(int(np.prod(U.shape[1:])), np.float64)
    for s in range(0, len(live), 1 << 16):  # (bounded float64 copies of U)
        idx = live[s:s + (1 << 16)]
        A += e[s:s + (1 << 16)] @ U[idx].reshape(len(idx), -1).astype(np.float64)
    return float(e.sum()), float((e * e).sum()), float((e * c).sum()), A
