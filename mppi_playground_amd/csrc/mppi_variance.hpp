// mppi_variance.hpp — Covariance adaptation (the sketch at mppi.py:400-418): the weighted, centred second moment of the clamped
// actions over the live noise tiles (weighted_variance_kernel) and the update of the per-step sigma table (sigma_update_kernel).
// Runs after steps 5-6 of a solve, only when the adaptation is switched on; see mppi_handle.hpp for the map of the files.
#pragma once
#include "mppi_covariance.hpp"
#include "mppi_reduce.hpp"

namespace mppi {

// ------------------------------------------------------------------------------------------
// var[t,k] * sum e = sum_i e_i * (U_i[t,k] - ubar[t,k])^2 with e_i = exp((-c_i)/lambda - (-c_min)/lambda) as in
// weights_reduce_kernel (the same fp32 expression, so the same weights to the bit), U_i = clamp(mean + eps_i) read from the
// materialised tiles and ubar = A / sum e from the solve's summary {min c, sum e, sum e^2, sum e*c, A[row]}: the weighted mean
// BEFORE the Savitzky-Golay step.  `mean` is the mean the solve sampled around, so the kernel runs before finalize stores
// the warm start.
//
// Phase A (per wave) is weights_reduce_kernel's: the costs of TPW tiles become weights and a bitmask of the tiles that carry
// any; tiles whose 64 weights are all exactly zero are skipped (exact: they add 0).  Phase B (per block): every live tile of
// the block is accumulated by all four waves, wave w taking the float4 groups r0 + w + 4m of this column chunk, so a column
// is owned by one wave and each lane adds fma(e, (u - ubar)^2, acc) in tile order.  Mean, clamp bounds and ubar come per
// COLUMN from LDS (bounds: the per-column table of wide handles, else u_min / u_max of column f % dim_control), so one code
// path serves every dim_control.  Blocks that saw a live tile publish one partial row and raise their flag; no atomics:
// sigma_update_kernel folds the rows in a fixed order, which makes the table bit-reproducible from run to run.
// Measured (racing N = 2^20, T = 50): 143 us with every tile live = 2.96 TB/s on the 424 MB it reads once,
// 0.37 of the HBM peak and 20 % behind weights_reduce_kernel on the same tiles; 8 us (launch latency) with one live tile.
// The groups are dealt statically (g = wid + 4m: a 25-group row gives wave 0 seven groups and the others six — the imbalance
// weights_reduce_kernel measured at 12 % and removed by spreading the remainder over the tiles) and every group reads four
// column tables from LDS; which of the two the 20 % is was not separated.  Kept simple: the path is opt-in.
// vpart layout: [gridDim.x][colsp], colsp = gridDim.y * 128; vlive: [gridDim.x].
__device__ __forceinline__ float variance_lane_sum8(float (*red)[WAVE + 1], const float* a8, int lane) {
    // lanes 0..7 return the sums over the wave of a8[0..7] (the transposed LDS sum of weights_reduce_kernel)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[j][lane] = a8[j];
    __builtin_amdgcn_wave_barrier();
    const float* rowp = &red[lane & 7][(lane >> 3) * 8];
    const float v0 = rowp[0] + rowp[1], v1 = rowp[2] + rowp[3], v2 = rowp[4] + rowp[5], v3 = rowp[6] + rowp[7];
    float v = (v0 + v1) + (v2 + v3);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    __builtin_amdgcn_wave_barrier();
    return v;
}

__global__ __launch_bounds__(BLOCK) void weighted_variance_kernel(const float4* __restrict__ noise,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ costs,
                                                                  const unsigned* __restrict__ min_key,
                                                                  const float* __restrict__ summary,
                                                                  const float* __restrict__ coltab,
                                                                  float* __restrict__ vpart, float* __restrict__ vlive,
                                                                  Dims d, float lambda_arg,
                                                                  const float* __restrict__ lambda_dev) {
    const float lambda = lambda_dev ? *lambda_dev : lambda_arg;
    constexpr int GPW = 8;
    constexpr int NACC = GPW * 4;
    constexpr int NW = BLOCK / WAVE;
    constexpr int CHG = NW * GPW;  // float4 groups per column chunk (weights_reduce_kernel's chunking)
    constexpr int TPW = 8;
    __shared__ float s_red[NW][8][WAVE + 1];
    __shared__ float s_e[NW][TPW][WAVE];
    __shared__ unsigned s_live[NW];
    // per column of this chunk: the mean and an all-zero copy (samples that do not inherit it), lo, hi, ubar
    __shared__ __attribute__((aligned(16))) float s_mean[2][CHG * 4];
    __shared__ __attribute__((aligned(16))) float s_col[3][CHG * 4];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.y * CHG;
    const float sum_e = summary[1];
    for (int j = threadIdx.x; j < CHG * 4; j += BLOCK) {
        const int f = 4 * r0 + j;
        const bool in = f < d.row;
        s_mean[0][j] = in ? mean[f] : 0.0f;
        s_mean[1][j] = 0.0f;
        s_col[0][j] = !in ? 0.0f : coltab ? coltab[4 * d.R + f] : d.u_min[f % d.dc];
        s_col[1][j] = !in ? 0.0f : coltab ? coltab[8 * d.R + f] : d.u_max[f % d.dc];
        s_col[2][j] = in ? summary[MPPI_SUMMARY_HEAD + f] / sum_e : 0.0f;  // finalize_tail's own quotient for one shard
    }
    const float cmin = key_to_float(*min_key);
    const float xmax = (-cmin) / lambda;
    float acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j) acc[j] = 0.0f;
    const int ng = min(CHG, d.R - r0);  // groups of the row in this chunk
    const int64_t nwaves = (int64_t)gridDim.x * NW;
    bool block_live = false;  // block-uniform
    for (int64_t base0 = (int64_t)blockIdx.x * NW; base0 < d.tiles; base0 += nwaves * TPW) {
        // ---- phase A: this wave's TPW tiles
        float cc[TPW];
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
            const int64_t i = (base0 + wid + q * nwaves) * 64 + lane;
            cc[q] = (i < d.N) ? costs[i] : INFINITY;  // tiles past the end have i >= N as well
        }
        unsigned live = 0;
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
            const float e = expf((-cc[q]) / lambda - xmax);  // exp(-inf) = 0 for the padding lanes
            const bool tile_live = __ballot(e != 0.0f) != 0ull;
            live |= (tile_live ? 1u : 0u) << q;
            if (tile_live) s_e[wid][q][lane] = e;  // wave-uniform
        }
        if (lane == 0) s_live[wid] = live;
        __syncthreads();  // (the first round's barrier also publishes the column tables)
        // ---- phase B: the block's live tiles, this wave's groups
        for (int w2 = 0; w2 < NW; ++w2) {
            const unsigned lv = __builtin_amdgcn_readfirstlane(s_live[w2]);
            if (lv == 0u) continue;
            block_live = true;
            for (int q = 0; q < TPW; ++q) {
                if (!((lv >> q) & 1u)) continue;
                const int64_t tile = base0 + w2 + q * nwaves;
                const int64_t i = tile * 64 + lane;
                const float e = s_e[w2][q][lane];
                const bool inherit = (d.sample_offset + i) < d.inherit_count;
                const float4* np = noise + (tile * d.R + r0) * 64 + lane;
                int moff = inherit ? 0 : CHG, coff = 0;  // float4 offsets into the column tables
                asm volatile("" : "+v"(moff), "+v"(coff));  // opaque: keeps the LDS reads inside the loop (see weights_reduce_kernel)
                const float4* mp = reinterpret_cast<const float4*>(&s_mean[0][0]) + moff;
                const float4* lop = reinterpret_cast<const float4*>(&s_col[0][0]) + coff;
                const float4* hp = reinterpret_cast<const float4*>(&s_col[1][0]) + coff;
                const float4* ubp = reinterpret_cast<const float4*>(&s_col[2][0]) + coff;
#pragma unroll
                for (int m = 0; m < GPW; ++m) {
                    const int g = wid + NW * m;  // group inside the chunk
                    if (g < ng) {                // wave-uniform
                        const float4 n4 = np[(int64_t)g * 64], m4 = mp[g], lo4 = lop[g], hi4 = hp[g], ub4 = ubp[g];
                        const float nv[4] = {n4.x, n4.y, n4.z, n4.w}, mv[4] = {m4.x, m4.y, m4.z, m4.w};
                        const float lo[4] = {lo4.x, lo4.y, lo4.z, lo4.w}, hi[4] = {hi4.x, hi4.y, hi4.z, hi4.w};
                        const float ub[4] = {ub4.x, ub4.y, ub4.z, ub4.w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float dev = clampf(mv[j] + nv[j], lo[j], hi[j]) - ub[j];
                            acc[4 * m + j] = fmaf(e, dev * dev, acc[4 * m + j]);
                        }
                    }
                }
            }
        }
        __syncthreads();  // s_e / s_live are rewritten by the next round
    }
    // cross-lane sums, 8 accumulators per pass; accumulator 4*m + j of wave w is column 4*(r0 + w + NW*m) + j of the row
    if (block_live) {  // (block-uniform)
        const int colsp = gridDim.y * CHG * 4;
#pragma unroll
        for (int p = 0; p < NACC / 8; ++p) {
            const float v = variance_lane_sum8(s_red[wid], &acc[p * 8], lane);
            const int a = p * 8 + lane;
            const int g = wid + NW * (a >> 2);
            if (lane < 8 && g < ng) vpart[(int64_t)blockIdx.x * colsp + 4 * (r0 + g) + (a & 3)] = v;
        }
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) vlive[blockIdx.x] = block_live ? 1.0f : 0.0f;
}

// ------------------------------------------------------------------------------------------
// One block: fold the published partial rows (ascending blocks; thread (c, g) sums rows g, g + 16, ... of column c0 + c
// in four interleaved accumulators, the 16 row groups are added in order), divide by sum e and move the table
// (covariance_step).  A voided solve (a temperature search that timed out leaves NaN weights) must not poison the table:
// a sum e that is not a positive finite number leaves every entry alone, a variance that is not finite leaves its own.
// sum e itself is never 0: the minimum-cost sample has e = 1.  lim = {sigma_min[dc], sigma_max[dc]}.
constexpr int SU_COLS = 64;
constexpr int SU_BLOCK = 1024;
__global__ __launch_bounds__(SU_BLOCK) void sigma_update_kernel(const float* __restrict__ vpart,
                                                                const float* __restrict__ vlive, int nblocks, int colsp,
                                                                int row, int dc, const float* __restrict__ summary,
                                                                const float* __restrict__ lim, float rate, float floor,
                                                                float* __restrict__ sigtab) {
    constexpr int NG = SU_BLOCK / SU_COLS;
    __shared__ float s_part[NG][SU_COLS + 1];
    __shared__ unsigned char s_live[REDUCE_MAX_BLOCKS];
    for (int b = threadIdx.x; b < nblocks; b += SU_BLOCK) s_live[b] = vlive[b] != 0.0f ? 1 : 0;
    const float sum_e = summary[1];
    if (!(sum_e > 0.0f) || !isfinite(sum_e)) return;  // (uniform)
    __syncthreads();
    const int c = threadIdx.x & (SU_COLS - 1), g = threadIdx.x / SU_COLS;
    for (int c0 = 0; c0 < row; c0 += SU_COLS) {
        const int f = c0 + c;
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (f < row) {
            for (int b = g; b < nblocks; b += 4 * NG) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int bb = b + q * NG;
                    if (bb < nblocks && s_live[bb]) a[q] += vpart[(int64_t)bb * colsp + f];
                }
            }
        }
        s_part[g][c] = (a[0] + a[1]) + (a[2] + a[3]);
        __syncthreads();
        if (g == 0 && f < row) {
            float v = 0.0f;
            for (int q = 0; q < NG; ++q) v += s_part[q][c];
            const float var = v / sum_e;
            if (isfinite(var)) {
                const int k = f % dc;
                const float s = sigtab[f];
                sigtab[f] = covariance_step(s * s, var, rate, floor, lim[k], lim[dc + k]);
            }
        }
        __syncthreads();
    }
}

}  // namespace mppi
