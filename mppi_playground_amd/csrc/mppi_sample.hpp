// mppi_sample.hpp — Step 1 (mppi.py:255-263): the device noise stream (gen_noise4 is its definition), sample_kernel, posterior
// draws, and their temporally correlated forms (sample_colored_kernel, posterior_colored_kernel).
// Part of the MPPI.forward() hot path for gfx950; see mppi_handle.hpp for the map of the files.
#pragma once
#include "mppi_colored.hpp"
#include "mppi_common.hpp"

namespace mppi {

// ------------------------------------------------------------------------------------------
// Step 1: eps ~ N(0, diag(sigma^2)).  gen_noise4() is THE definition of the device noise: float4
// group r of global sample gi.  It is used by sample_kernel (materialise the lane-major tiles) and,
// in "regen" mode, directly by the rollout and reduction kernels, which then never touch HBM for
// the noise (Philox + Box-Muller is ~25 VALU per normal, cheaper than a 16 B/lane HBM round trip).
// WIDE (generic handles whose dim_control is not 1, 2 or 4): the control index of a flat column depends on the
// group, so sigma / bounds come from the per-column table `coltab` = {sigma[4R], lo[4R], hi[4R]} (built on the host,
// zeros past the row) instead of the launch constants in Dims.
// The two halves of gen_noise4 (the integer hash and the Box-Muller transform of its output), separately callable so
// that the rollout loop can run them one group apart (software pipeline: see trajectory_cost).
__device__ __forceinline__ u32x4 noise_bits(uint64_t gi, int r, const GenCtx& g) {
    return philox4x32_10((uint32_t)gi, (uint32_t)(gi >> 32), (uint32_t)r, g.solve_idx, g.seed_lo, g.seed_hi);
}
template <bool WIDE = false>
__device__ __forceinline__ float4 noise_from_bits(const u32x4& x, int r, const Dims& d,
                                                  const float* __restrict__ sig_cols = nullptr) {
    float z[4];
    box_muller(x.x, x.y, z[0], z[1]);
    box_muller(x.z, x.w, z[2], z[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] *= WIDE ? sig_cols[4 * r + j] : d.sigma[ctrl_index(j, d.dc)];
    return make_float4(z[0], z[1], z[2], z[3]);
}
struct KeyPins { uint32_t k0v, k1v, k0w; };  // key words in VGPRs (philox4x32_10: rounds 0 and 1), pinned once by a caller with a hot loop
// U1_FMA: which of box_muller's two equal forms of u1 the caller's registers afford (philox.hpp).
template <bool WIDE = false, bool U1_FMA = true>
__device__ __forceinline__ float4 gen_noise4(uint64_t gi, int r, const GenCtx& g, const Dims& d,
                                             const float* __restrict__ sig_cols = nullptr, const KeyPins* pins = nullptr) {
    const u32x4 x = philox4x32_10((uint32_t)gi, (uint32_t)(gi >> 32), (uint32_t)r, g.solve_idx, g.seed_lo, g.seed_hi,
                                  pins ? pins->k0v : g.seed_lo, pins ? pins->k1v : g.seed_hi,
                                  pins ? pins->k0w : g.seed_lo + 0x9E3779B9u);
    float z[4];
    box_muller<U1_FMA>(x.x, x.y, z[0], z[1]);
    box_muller<U1_FMA>(x.z, x.w, z[2], z[3]);
    // columns past the row length (row % 4 != 0) carry unused values: no consumer reads them
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] *= WIDE ? sig_cols[4 * r + j] : d.sigma[ctrl_index(j, d.dc)];
    return make_float4(z[0], z[1], z[2], z[3]);
}

// HBM-write bound: 16 B per lane per Philox call, one 1 KiB store per wave instruction.
template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void sample_kernel(float4* __restrict__ noise, Dims d, GenCtx g,
                                                       const float* __restrict__ coltab) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6);
    if (tile >= d.tiles) return;
    const uint64_t gi = (uint64_t)(d.sample_offset + tile * 64 + lane);
    float4* out = noise + tile * d.R * 64 + lane;
    for (int r = 0; r < d.R; ++r) out[(int64_t)r * 64] = gen_noise4<WIDE>(gi, r, g, d, coltab);
}

// get_samples_from_posterior (mppi.py:489-506): samples[q][f] = loc[f] + eps_q[f] with eps ~ N(0, diag(sigma^2)) from
// the Philox stream of a solve index RESERVED for this call (counter = (q, group, solve_idx): the draw advances the
// solver's stream exactly like a forward() would, and every shard draws the same k samples).  Unclamped, like the
// reference's MultivariateNormal(loc=optimal_solution).sample().  One thread per (sample, float4 group).
template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void posterior_sample_kernel(const float* __restrict__ loc, int k,
                                                                 float* __restrict__ samples, Dims d, GenCtx g,
                                                                 const float* __restrict__ coltab) {
    const int64_t idx = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= (int64_t)k * d.R) return;
    const int q = (int)(idx / d.R), r = (int)(idx - (int64_t)q * d.R);
    const float4 n4 = gen_noise4<WIDE>((uint64_t)q, r, g, d, coltab);
    const float nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = 4 * r + j;
        if (f < d.row) samples[(int64_t)q * d.row + f] = loc[f] + nv[j];
    }
}

// ------------------------------------------------------------------------------------------
// Temporally correlated noise (opt-in, mppi_set_noise_correlation; mppi_colored.hpp is the scalar rule): the standard normals
// of one (sample, control dimension) run through z[t] = beta[k] z[t-1] + alpha[k] xi[t] along the horizon, z[0] = xi[0],
// and only then meet sigma: eps[i][t][k] = z[t] * s[t][k].  xi is what gen_noise4 draws before its multiplication by sigma,
// same counters, so the filtered and the unfiltered stream of one seed consume the same normals.  Column f = 4r + j of the
// row is step f / dc of dimension f % dc: the filter links column f to column f - dc, inside a float4 group as well as
// across groups.  sigma, beta and alpha come per column from tables of 4R entries built on the host (zeros past the row:
// those columns come out as 0), wave-uniform reads, one code path for every dim_control.
__device__ __forceinline__ void gen_normal4(uint64_t gi, int r, const GenCtx& g, float (&z)[4]) {
    const u32x4 x = noise_bits(gi, r, g);
    box_muller(x.x, x.y, z[0], z[1]);
    box_muller(x.z, x.w, z[2], z[3]);
}
// dim_control <= 4: `carry` holds the filtered normals of the last DC columns, oldest first (registers; starts as zeros).
// z: xi of group r on entry, the filtered normals on return.  `coef` = {beta[C], alpha[C]}, C = 4R.
template <int DC>
__device__ __forceinline__ void colored_group_carry(float (&z)[4], int r, const float* __restrict__ coef, int C, float (&carry)[DC]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = 4 * r + j;
        const float zn = f < DC ? z[j] : colored_step(carry[0], z[j], coef[f], coef[C + f]);
#pragma unroll
        for (int i = 0; i + 1 < DC; ++i) carry[i] = carry[i + 1];
        carry[DC - 1] = zn;
        z[j] = zn;
    }
}
// dim_control > 4: column f - dc lies in an earlier group, which the caller has stored already; `earlier(f)` reads it back.
template <class Earlier>
__device__ __forceinline__ void colored_group_readback(float (&z)[4], int r, int dc, const float* __restrict__ coef, int C, Earlier earlier) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = 4 * r + j;
        if (f >= dc) z[j] = colored_step(earlier(f - dc), z[j], coef[f], coef[C + f]);
    }
}

// sample_kernel's geometry and store pattern (one lane per trajectory, one wave per tile, lane-major 1 KiB stores); the lane
// walks its groups in order and carries the filter.  DC = dim_control for 1..4.  DC = 0 is every wider row: the lane stores
// its FILTERED NORMALS first and reads column f - dc back from the tile it has just written — the same thread loading from
// the address it stored to, which a thread always sees in program order, so no fence or barrier is needed — and scales the
// row by sigma in a second walk (the scaled value fl(z * s) would not give z back).
template <int DC>
__global__ __launch_bounds__(BLOCK) void sample_colored_kernel(float4* noise, Dims d, GenCtx g, const float* __restrict__ sig_cols,
                                                               const float* __restrict__ coef) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6);
    if (tile >= d.tiles) return;
    const uint64_t gi = (uint64_t)(d.sample_offset + tile * 64 + lane);
    float4* out = noise + tile * d.R * 64 + lane;
    const int C = 4 * d.R;
    float z[4];
    if constexpr (DC > 0) {
        float carry[DC] = {};
        for (int r = 0; r < d.R; ++r) {
            gen_normal4(gi, r, g, z);
            colored_group_carry<DC>(z, r, coef, C, carry);
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] *= sig_cols[4 * r + j];
            out[(int64_t)r * 64] = make_float4(z[0], z[1], z[2], z[3]);
        }
    } else {
        const auto earlier = [out](int f) {
            const float4 p = out[(int64_t)(f >> 2) * 64];
            const int j = f & 3;
            return j == 0 ? p.x : j == 1 ? p.y : j == 2 ? p.z : p.w;
        };
        for (int r = 0; r < d.R; ++r) {
            gen_normal4(gi, r, g, z);
            colored_group_readback(z, r, d.dc, coef, C, earlier);
            out[(int64_t)r * 64] = make_float4(z[0], z[1], z[2], z[3]);
        }
        for (int r = 0; r < d.R; ++r) {
            const float4 p = out[(int64_t)r * 64];
            const float* s = sig_cols + 4 * r;
            out[(int64_t)r * 64] = make_float4(p.x * s[0], p.y * s[1], p.z * s[2], p.w * s[3]);
        }
    }
}

// posterior_sample_kernel through the same filter: one thread per sample walks its row (k is small).  DC as above; the wide
// form keeps the filtered normals in the sample's own output row until its second walk.
template <int DC>
__global__ __launch_bounds__(BLOCK) void posterior_colored_kernel(const float* __restrict__ loc, int k, float* samples, Dims d, GenCtx g,
                                                                  const float* __restrict__ sig_cols, const float* __restrict__ coef) {
    const int q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= k) return;
    float* row = samples + (int64_t)q * d.row;
    const int C = 4 * d.R;
    float z[4];
    if constexpr (DC > 0) {
        float carry[DC] = {};
        for (int r = 0; r < d.R; ++r) {
            gen_normal4((uint64_t)q, r, g, z);
            colored_group_carry<DC>(z, r, coef, C, carry);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = 4 * r + j;
                if (f < d.row) row[f] = loc[f] + z[j] * sig_cols[f];
            }
        }
    } else {
        const auto earlier = [row](int f) { return row[f]; };  // (f - dc < row for every column of the 4R, dc > 4)
        for (int r = 0; r < d.R; ++r) {
            gen_normal4((uint64_t)q, r, g, z);
            colored_group_readback(z, r, d.dc, coef, C, earlier);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * r + j < d.row) row[4 * r + j] = z[j];
        }
        for (int f = 0; f < d.row; ++f) row[f] = loc[f] + row[f] * sig_cols[f];
    }
}

// One float4 group of a lane's noise row: from the tiles (GEN=false) or regenerated (GEN=true).
template <bool GEN, bool U1_FMA = true>
__device__ __forceinline__ float4 noise_group(const float4* __restrict__ np, int r, uint64_t gi, const GenCtx& g,
                                              const Dims& d, const KeyPins* pins = nullptr) {
    if (GEN) return gen_noise4<false, U1_FMA>(gi, r, g, d, nullptr, pins);
    return np[(int64_t)r * 64];
}

}  // namespace mppi
