"""Cases for solve_fused_kernel (the single-launch solve): the host's block geometry restated, the tables of sample counts and
row shapes, where a single weighted sample is placed, the float64 reference of the sums over the kernel's own partition of
the exponent, and the longest fp32 addition chain of a column.

Nothing here touches the GPU or the library.  tests/test_fused_cases_host.py asserts that the tables reach what they claim;
tests/test_gpu_fused_geometry.py runs them.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
WAVE = 64
FUSED_BLOCK = 512                # threads per block = the most trajectories a block owns
FUSED_MAX_BLOCKS = 256
FUSED_MAX_ROW = 128
FUSED_SMALL_BLOCKS = 32          # up to this many blocks a block's exponents are relative to its OWN minimum
FX_CELLS = FUSED_MAX_ROW + 8
STATS_L = 32
RPARTS = FUSED_BLOCK // FX_CELLS                 # 3 row groups of the row fold
SPARTS = FUSED_BLOCK // (STATS_L * 3)            # 5 row groups of the statistics combine
KS = -(-FUSED_SMALL_BLOCKS // RPARTS)            # 11 cells per thread with few blocks
KG = 32                                          # cells per thread and pass beyond
AUTO_MAX_SAMPLES = 4096          # "fused_solve" = 1 with a fixed temperature or MPO
AUTO_MAX_SAMPLES_SEARCH = 16384  # ... under ESSPS, or LBPS on grids


def _cdiv(a, b):
    return -(-int(a) // int(b))


# ------------------------------------------------------------------------------ launch geometry
def geometry(N, cu=256, search=False, mode=1, row=1):
    """(G, spb) of the single launch, or None where mppi_solve takes the multi-kernel path (capi_solve.hip: fused_applies and
    solve_fused).  `mode` is the option "fused_solve", `search` says that ESSPS or LBPS-on-grids runs on the device, `row` is
    T * dim_control."""
    gmax = min(FUSED_MAX_BLOCKS, int(cu))
    if mode == 0 or row > FUSED_MAX_ROW or N > FUSED_BLOCK * gmax:
        return None
    if mode == 1 and N > (AUTO_MAX_SAMPLES_SEARCH if search else AUTO_MAX_SAMPLES):
        return None
    grid0 = max(1, min(gmax, _cdiv(N, WAVE)))
    if N <= AUTO_MAX_SAMPLES:
        grid0 = min(grid0, FUSED_SMALL_BLOCKS)
    spb = WAVE * _cdiv(_cdiv(N, grid0), WAVE)
    return _cdiv(N, spb), spb


def row_shape(T, dc):
    """(R, RP): float4 groups of the row and their count rounded up to a power of two (mppi_fused.hpp: `while (RP < d.R)`)."""
    R = _cdiv(T * dc, 4)
    RP = 1
    while RP < R:
        RP <<= 1
    return R, RP


# ------------------------------------------------------------------------------ the tables
SIZE_T = 5          # pendulum: row 5, two float4 groups, the second one quarter used
# N -> what it is there for (cu = 256)
SIZES = [
    (1, "one lane"), (64, "one full wave"), (65, "second block holds one lane"),
    (2048, "G = 32, spb = 64"), (2049, "G = 17, spb = 128, last block one lane and an empty second wave"),
    (4096, "G = 32, spb = 128: the largest own-minimum grid"),
    (4097, "G = 65: the first grid with the minimum hop"), (6145, "G = 97: second pass of the b0 += KG * RPARTS loop"),
    (16384, "G = 256, spb = 64"), (16385, "G = 129, spb = 128"),
    (255 * 192 + 1, "spb = 192"), (255 * 256 + 1, "spb = 256"), (255 * 320 + 1, "spb = 320"), (255 * 384 + 1, "spb = 384"),
    (255 * 448 + 1, "spb = 448"),
    (130561, "spb = 512, last block one lane, seven empty waves"), (131072, "the largest size the kernel accepts"),
]
SIZE_NS = [n for n, _ in SIZES]
ROW_TABLE_N = 1000  # G = 16, spb = 64
ROW_TABLE = ([("pendulum", T) for T in (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 32, 33, 64, 65, 127, 128)]
             + [("nav2d", T) for T in (2, 3, 9, 33, 64)])
ROW_TOO_WIDE = ("pendulum", 129)   # row 129 > FUSED_MAX_ROW: the multi-kernel path takes it
DIM_CONTROL = {"pendulum": 1, "nav2d": 2}
EXPLORATION = 0.3


def fused_mode(N):
    """The "fused_solve" option a fixed-temperature case of N samples runs under."""
    return 2 if N > AUTO_MAX_SAMPLES else 1


def inherit_count(N, exploration=EXPLORATION):
    return int(N * (1 - exploration))   # (pi_mpc/mppi.py)


def split_inside_a_block(N, cu=256):
    """The exploration split of EXPLORATION falls strictly inside a block: samples on both sides of it share a block."""
    g = geometry(N, cu, mode=fused_mode(N))
    k = inherit_count(N)
    return g is not None and 0 < k < N and k % g[1] != 0


def _lane_in(block, N, spb):
    """A lane of `block` away from the block's edges, different from block to block."""
    have = min(spb, N - block * spb)
    return block * spb + (37 * block + 5) % have


def targets(N, G, spb):
    """Local sample indices at which the only weighted sample is placed: the edges of waves and blocks, both ends of the last
    two blocks, and one lane in the blocks on both sides of the folds' loop edges (own-minimum path: thread 0 of the row fold
    sums blocks 0, 3, ..., 30, KS = 11 of them; beyond: the second pass starts at block KG * RPARTS = 96).  Clipped to what
    exists, without duplicates, ascending."""
    want = [0, 63, 64, spb - 1, spb, N - 1, (G - 1) * spb, (G - 1) * spb - 1]
    for b in ((10, 11, 30, 31) if G <= FUSED_SMALL_BLOCKS else (95, 96, 97, 255)):
        if b < G:
            want.append(_lane_in(b, N, spb))
    return sorted({int(i) for i in want if 0 <= i < N})


# ------------------------------------------------------------------------------ the reference
def _fdiv(a, lam):
    return (np.asarray(a, f32) / f32(lam)).astype(f32)


def weights(costs, lam, G, spb, search=False):
    """float64 un-normalised weights from the fp32 argument the kernel forms; exp and everything after it in float64.
    More than FUSED_SMALL_BLOCKS blocks, or a temperature search (every block has seen all minima by the time it weighs):
    fl(fl(-c / lam) - fl(-c_min / lam)).  Otherwise per block b, relative to its own minimum c_ref,b:
    exp(fl(fl(-c / lam) - fl(-c_ref,b / lam))) * exp(fl(fl(-c_ref,b / lam) - fl(-c_min / lam)))."""
    c = np.asarray(costs, f32)
    N = len(c)
    cmin = c.min()
    xmin = _fdiv(-cmin, lam)
    if G > FUSED_SMALL_BLOCKS or search:
        return np.exp((_fdiv(-c, lam) - xmin).astype(f32).astype(np.float64))
    e = np.empty(N, np.float64)
    for b in range(G):
        lo, hi = b * spb, min(N, (b + 1) * spb)
        xref = _fdiv(-c[lo:hi].min(), lam)
        scale = np.exp(np.float64(f32(xref - xmin)))
        e[lo:hi] = np.exp((_fdiv(-c[lo:hi], lam) - xref).astype(f32).astype(np.float64)) * scale
    return e


def reference(U, costs, lam, G, spb, search=False):
    """(c_min, sum e, sum e^2, sum e*c, A[row]) in float64 from `weights`; samples of weight 0 are left out.
    A = sum_i e_i U_i is the un-normalised row."""
    e = weights(costs, lam, G, spb, search)
    c = np.asarray(costs, f32)
    live = np.nonzero(e != 0.0)[0]
    e, cl = e[live], c[live].astype(np.float64)
    U = np.asarray(U)
    A = np.zeros(int(np.prod(U.shape[1:])), np.float64)
    for s in range(0, len(live), 1 << 16):  # (bounded float64 copies of U)
        idx = live[s:s + (1 << 16)]
        A += e[s:s + (1 << 16)] @ U[idx].reshape(len(idx), -1).astype(np.float64)
    return float(c.min()), float(e.sum()), float((e * e).sum()), float((e * cl).sum()), A


def scales(U, costs, e):
    """(sum e |c|, sum_i e_i |U_i| [row]): what an error of a signed sum is measured against."""
    c = np.abs(np.asarray(costs, f32).astype(np.float64))
    live = np.nonzero(e != 0.0)[0]
    U = np.asarray(U)
    S = np.zeros(int(np.prod(U.shape[1:])), np.float64)
    for s in range(0, len(live), 1 << 16):
        idx = live[s:s + (1 << 16)]
        S += e[idx] @ np.abs(U[idx].reshape(len(idx), -1).astype(np.float64))
    return float((e[live] * c[live]).sum()), S


# ------------------------------------------------------------------------------ the limit
def chain(G, spb, R):
    """The longest sequential fp32 addition chain of a row column through the kernel: a thread's slice loop over its block's
    samples, the two-step slice fold staged in s_p (nsl / Q slices, then the Q groups), the block fold of one row group
    (at most KS fused steps with few blocks, ceil(G / RPARTS) additions beyond) and the RPARTS row groups."""
    RP = 1
    while RP < R:
        RP <<= 1
    nsl = FUSED_BLOCK // RP
    Q = FUSED_BLOCK // (4 * RP)
    fold = min(KS, _cdiv(G, RPARTS)) if G <= FUSED_SMALL_BLOCKS else _cdiv(G, RPARTS)
    return _cdiv(spb, nsl) + nsl // Q + Q + fold + RPARTS


def limit(G, spb, R, tol=1e-5):
    return max(tol, chain(G, spb, R) * 2.0 ** -24)
