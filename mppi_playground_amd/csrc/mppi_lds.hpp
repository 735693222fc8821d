// mppi_lds.hpp — the dynamic-LDS layout of every kernel that carves regions out of `extern __shared__`: one struct per
// kernel, with the offset (in floats) of each region and floats(), the total the launch site asks for.  The kernel takes its
// offsets from here and the launch site its size, so the two cannot drift apart (a drift would be an LDS overrun, not a
// failing test).  Static constexpr functions of explicit scalars only: a kernel that calls one compiles to what the
// written-out expression compiled to.  Where a kernel keeps a written-out expression (another unit of address, another
// association of the sum), a comment there names the function it mirrors.
// Plain C++ as well as HIP: tests/host_emul/lds_layouts.cpp checks order, alignment and totals with g++.
#pragma once
#include <cstddef>

#include "../../include/mppi_hip.h"

#ifdef __HIPCC__
#define MPPI_LDS_FN __host__ __device__
#else
#define MPPI_LDS_FN
#endif

namespace mppi {

// Savitzky-Golay staging of finalize_tail: [history (T-1); action (T)] per control dimension, padded by window/2 at both ends
MPPI_LDS_FN constexpr int sg_staging_floats(int T, int dc, int window) {
    return window ? (2 * T - 1 + 2 * (window / 2)) * dc : 0;
}

// rollout_cost_kernel / rollout_action_cost_kernel (`ac`: with the control-cost term): [4R] mean groups, [4R] zeros (samples
// that do not inherit the mean), (ac: [4R] g = mean * inverse covariance,) [T * krow] step rows.  The one extra block that
// rides a pending state sequence uses the same memory as [row] action, [ds <= MPPI_MAX_DIM_STATE] start state.
struct RolloutLds {
    MPPI_LDS_FN static constexpr int mean() { return 0; }
    MPPI_LDS_FN static constexpr int zeros(int R) { return 4 * R; }
    MPPI_LDS_FN static constexpr int g(int R) { return 8 * R; }
    MPPI_LDS_FN static constexpr int ktab(int R, bool ac) { return (ac ? 12 : 8) * R; }
    MPPI_LDS_FN static constexpr int rider_act() { return 0; }
    MPPI_LDS_FN static constexpr int rider_x0(int row) { return row; }
    MPPI_LDS_FN static constexpr size_t floats(int R, int T, int row, int krow, bool ac) {
        const size_t lanes = (size_t)(ac ? 12 : 8) * R + (size_t)T * krow, rider = (size_t)row + MPPI_MAX_DIM_STATE;
        return lanes > rider ? lanes : rider;
    }
};

// solve_fused_kernel: [4R] mean groups, [4R] zeros, [T * krow] step rows, then block 0's tail: [row] action, [4 + row] summary,
// the filter staging
struct FusedLds {
    MPPI_LDS_FN static constexpr int mean() { return 0; }
    MPPI_LDS_FN static constexpr int zeros(int R) { return 4 * R; }
    MPPI_LDS_FN static constexpr int ktab(int R) { return 8 * R; }
    MPPI_LDS_FN static constexpr int act(int R, int T, int krow) { return 8 * R + T * krow; }
    MPPI_LDS_FN static constexpr int sum(int R, int T, int row, int krow) { return act(R, T, krow) + row; }
    MPPI_LDS_FN static constexpr int yp(int R, int T, int row, int krow) { return sum(R, T, row, krow) + MPPI_SUMMARY_HEAD + row; }
    MPPI_LDS_FN static constexpr size_t floats(int R, int T, int row, int dc, int krow, int window) {
        return (size_t)8 * R + (size_t)T * krow + 2 * (size_t)row + MPPI_SUMMARY_HEAD + (size_t)sg_staging_floats(T, dc, window);
    }
};

// finalize_kernel: [row] action, [world][4 + row] own / collected summaries, the filter staging and — when the kernel folds
// the partial rows itself — [FOLD_GROUPS][row + 3] group sums (summarize_kernel's tree)
struct FinalizeLds {
    static constexpr int FOLD_GROUPS = 64;
    MPPI_LDS_FN static constexpr int act() { return 0; }
    MPPI_LDS_FN static constexpr int sum(int row) { return row; }
    MPPI_LDS_FN static constexpr int yp(int row, int world) { return sum(row) + world * (MPPI_SUMMARY_HEAD + row); }
    MPPI_LDS_FN static constexpr int fold(int T, int row, int dc, int world, int window) {
        return yp(row, world) + sg_staging_floats(T, dc, window);
    }
    MPPI_LDS_FN static constexpr size_t floats(int T, int row, int dc, int world, int window, bool fold) {
        return (size_t)row + (size_t)world * (row + MPPI_SUMMARY_HEAD) + (size_t)sg_staging_floats(T, dc, window) +
               (fold ? (size_t)FOLD_GROUPS * (row + 3) : 0);
    }
};

// state_seq_kernel: [row] action, [ds] start state (what finalize_kernel left in b1); sized for MPPI_MAX_DIM_STATE
struct StateSeqLds {
    MPPI_LDS_FN static constexpr int act() { return 0; }
    MPPI_LDS_FN static constexpr int x0(int row) { return row; }
    MPPI_LDS_FN static constexpr size_t floats(int row) { return (size_t)row + MPPI_MAX_DIM_STATE; }
};

// rollout_cost_wave_kernel: per wave of the block, [4R] U then [(T + 1) * ds] S
struct WaveRolloutLds {
    static constexpr int WAVES = 4;  // waves per block
    MPPI_LDS_FN static constexpr int per_wave(int R, int T, int ds) { return 4 * R + (T + 1) * ds; }
    MPPI_LDS_FN static constexpr int u() { return 0; }
    MPPI_LDS_FN static constexpr int s(int R) { return 4 * R; }
    MPPI_LDS_FN static constexpr size_t floats(int R, int T, int ds) { return WAVES * ((size_t)4 * R + (size_t)(T + 1) * ds); }
};

// topk_rollout_kernel: [4R] the mean row the solve sampled around, [4R] zeros, then — unsorted candidates whose noise is
// regenerated (`gen`), rows of up to PREGEN_MAX_R groups — the block's noise, [R][64] float4
struct TopkLds {
    static constexpr int PREGEN_MAX_R = 32;  // rows of up to 32 float4 groups (T <= 64 at two controls): 32 KiB of LDS
    MPPI_LDS_FN static constexpr int mean() { return 0; }
    MPPI_LDS_FN static constexpr int zeros(int R) { return 4 * R; }
    MPPI_LDS_FN static constexpr int noise(int R) { return 8 * R; }
    MPPI_LDS_FN static constexpr bool pregen(int R, bool sorted, bool gen) { return !sorted && gen && R <= PREGEN_MAX_R; }
    MPPI_LDS_FN static constexpr size_t floats(int R, bool sorted, bool gen) {
        return 8 * (size_t)R + (pregen(R, sorted, gen) ? 4 * 64 * (size_t)R : 0);
    }
};

// lbps_brent_kernel: the block's costs, [per_thread][threads], when they are staged at all
struct BrentStageLds {
    MPPI_LDS_FN static constexpr int cost() { return 0; }
    MPPI_LDS_FN static constexpr size_t floats(int per_thread, int threads) { return (size_t)per_thread * threads; }
};

}  // namespace mppi
