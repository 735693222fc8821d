// mppi_particles.hpp — risk-aware solves (include/mppi_hip.h: mppi_set_particles): rollout_particles_kernel rolls every sample
// out from every one of P start states into a [P][N] cost matrix, particle_fold_kernel folds the P costs of a sample into one.
// Both are launched by capi_particles.hip only; see mppi_handle.hpp for the map of the files.
#pragma once
#include "mppi_rollout.hpp"

namespace mppi {

// ------------------------------------------------------------------------------------------
// Steps 1b-3 (mppi.py:266-336) from P start states: the unit of work is a (tile, particle) pair — a wave walks one tile of 64
// samples from one particle — on a grid of ceil(tiles / 4) x P blocks, the particle on blockIdx.y.  The wave calls lane_cost as
// rollout_cost_kernel does, with x0 = particles + m * DS: what lane_cost decides from the start state (the copy of the loop for
// a start outside the position clamp, racing's unit wheel base, the library-math redo of a lane that left a fast path) is
// decided per particle, and the cost of (i, m) is what the plain kernel computes for sample i from that state, bit for bit.
// The noise of a sample does not depend on the particle: every particle's wave regenerates (GEN) or reads the same groups.
// LDS as rollout_cost_kernel stages it (RolloutLds without the control-cost rows: that term does not depend on the state and
// is added once, behind the fold).  Block (0, 0) writes the snapshots the plain kernel's block 0 writes: x0_used takes the
// NOMINAL state (later re-rolls and finalize's state sequence start there), mean_used the mean.  No rider block, no stamps:
// the stage is timed on its two dispatches.  The minimum key belongs to the fold.
// The learned-dynamics models (the MLP ids only, behind `if constexpr`: every other instantiation is the text above) may
// carry particle m through ensemble member members[m] (mppi_set_particle_members): the launch site hands the members'
// offsets into the weight buffer in ctx.pad (mppi_models.hpp: member_offsets), the block reads its entry at a uniform address
// and moves ITS copy of ctx.ref.  The cost of (i, m) is then what a plain handle holding that member's table computes.
template <int MODEL, int FAST, bool GEN, bool UC, bool TRACK = false>
__global__ __launch_bounds__(BLOCK) void rollout_particles_kernel(const float4* __restrict__ noise,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ particles,
                                                                  const float* __restrict__ x0_nominal,
                                                                  float* __restrict__ pcosts,
                                                                  float* __restrict__ mean_used,
                                                                  float* __restrict__ x0_used, Dims d, GenCtx gen,
                                                                  ModelCtx ctx) {
    using M = ModelT<MODEL, FAST>;
    // the row of the matrix this block writes waits for the end of the horizon loop in LDS, not in a pair of SGPRs held across
    // it (rollout_cost_kernel says what live SGPRs cost there)
    __shared__ float* s_out;
    const int m = blockIdx.y;
    const bool first = blockIdx.x == 0 && m == 0;
    if (threadIdx.x == 0) s_out = pcosts + (int64_t)m * d.N;
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];  // RolloutLds: [4R] mean groups, [4R] zeros, [T * KROW] step rows
    if (first && threadIdx.x < M::DS) x0_used[threadIdx.x] = x0_nominal[threadIdx.x];
    float4* s_mean4 = reinterpret_cast<float4*>(s_dyn);
    float* s_ktab = s_dyn + RolloutLds::ktab(d.R, false);
    for (int f = threadIdx.x; f < 4 * d.R; f += BLOCK) {
        const float v = f < d.row ? mean[f] : 0.0f;
        s_dyn[f] = v;
        s_dyn[RolloutLds::zeros(d.R) + f] = 0.0f;
        if (first && f < d.row) mean_used[f] = v;
    }
    for (int f = threadIdx.x; f < d.T * M::KROW; f += BLOCK) s_ktab[f] = ctx.ref[f];
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * (BLOCK / WAVE) + wid;
    if (tile >= d.tiles) return;
    const int64_t i = tile * 64 + lane;
    const uint64_t gi = (uint64_t)(d.sample_offset + i);
    const bool inherit = (d.sample_offset + i) < d.inherit_count;
    const float4* np = noise + tile * d.R * 64 + lane;
    const float4* mp = inherit ? s_mean4 : s_mean4 + d.R;  // (RolloutLds::zeros, in float4 groups)
    if constexpr (is_mlp(MODEL)) {
        // a member per particle: the block's copy of the table pointer moves to its member's table (the step reads it through
        // the constant address space: scalar loads, as before).  No map: ctx.pad is null and the pointer stays where it was.
        ModelCtx mctx = ctx;
        if (ctx.pad != nullptr) mctx.ref = ctx.ref + member_offsets(ctx)[m];
        const float total = lane_cost<MODEL, FAST, GEN, UC, false, TRACK>(np, gi, gen, mp, s_ktab, particles + m * M::DS, d, mctx);
        if (i < d.N) s_out[i] = total;
    } else {
        const float total = lane_cost<MODEL, FAST, GEN, UC>(np, gi, gen, mp, s_ktab, particles + m * M::DS, d, ctx);
        if (i < d.N) s_out[i] = total;
    }
}

// ------------------------------------------------------------------------------------------
// The fold (include/mppi_hip.h has the arithmetic): one lane per sample, the P costs of the sample in registers.  MEAN and
// WORST are one pass; CVAR orders the values from largest to smallest with a fixed compare-exchange network (odd-even
// transposition: P rounds of neighbour exchanges, max to the front — P is a template argument, so the network is straight-line
// code on registers) and adds the first k in that order.  Every operation rounds on its own (the unit is compiled with FP
// contraction off) and the division is the IEEE quotient.  A NaN among the P values makes the folded cost NaN.
// Writes costs[i] and accumulates the minimum into the double-buffered key as the rollout kernels do: atomicMin into `min_key`
// (reset by the launch before), block 0 resets the other slot for the next launch.  The kernel is bound by memory, not by
// arithmetic, so the one atomic per block shows: at most FOLD_MAX_BLOCKS blocks stride over the samples (4096 blocks at
// N = 2^20 spent 50 us, mostly queueing at the key's address), and a block whose minimum is not below what the key already
// holds skips the atomic (the key only ever falls, so a stale read errs on the side of one atomic too many).
constexpr int FOLD_MAX_BLOCKS = 1024;
template <int P>
__global__ __launch_bounds__(BLOCK) void particle_fold_kernel(const float* __restrict__ pcosts, float* __restrict__ costs,
                                                              unsigned* __restrict__ min_key,
                                                              unsigned* __restrict__ next_min_key, int64_t N, int mode,
                                                              int k) {
    __shared__ float s_min[BLOCK / WAVE];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) *next_min_key = 0xFFFFFFFFu;
    float total = INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * BLOCK) {
        float c[P];
        bool nan = false;
#pragma unroll
        for (int m = 0; m < P; ++m) {
            c[m] = pcosts[(int64_t)m * N + i];
            nan = nan || c[m] != c[m];
        }
        float a = c[0];
        if (mode == MPPI_RISK_WORST) {
#pragma unroll
            for (int m = 1; m < P; ++m) a = fmaxf(a, c[m]);
        } else if (mode == MPPI_RISK_CVAR) {
#pragma unroll
            for (int round = 0; round < P; ++round) {
#pragma unroll
                for (int j = round & 1; j + 1 < P; j += 2) {
                    const float hi = fmaxf(c[j], c[j + 1]), lo = fminf(c[j], c[j + 1]);
                    c[j] = hi;
                    c[j + 1] = lo;
                }
            }
            a = c[0];
#pragma unroll
            for (int j = 1; j < P; ++j) a = j < k ? a + c[j] : a;
            a = a / (float)k;
        } else {
#pragma unroll
            for (int m = 1; m < P; ++m) a = a + c[m];
            a = a / (float)P;
        }
        const float folded = nan ? __builtin_nanf("") : a;
        costs[i] = folded;
        total = fminf(total, folded);
    }
    const float wm = wave_min(total);
    if (lane == 0) s_min[wid] = wm;
    __syncthreads();
    if (threadIdx.x == 0) {
        float mn = s_min[0];
#pragma unroll
        for (int w = 1; w < BLOCK / WAVE; ++w) mn = fminf(mn, s_min[w]);
        if (mn < INFINITY && float_to_key(mn) < *(volatile unsigned*)min_key) atomicMin(min_key, float_to_key(mn));
    }
}

}  // namespace mppi
