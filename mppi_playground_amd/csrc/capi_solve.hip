// capi_solve.hip — C ABI (include/mppi_hip.h): the solve — noise, rollout + costs, weights + reduction, finalize, the lazily
// completed state sequence, the single-launch solve and mppi_solve, which chains them.  The whole hot path is this one unit
// (only the device-resident temperature searches live in capi_search.hip).
#include <cmath>

#include "mppi_handle.hpp"
#include "mppi_layout.hpp"

namespace mppi {

// Sum the per-block partial rows into the shard summary {min c, sum e, sum e^2, sum e*c, A[row]}.  Only blocks
// that saw a live tile published a row (heads[b][3]); every block of this kernel first compacts the ascending
// list of those rows, then thread (c = tid & 15, g = tid >> 4) of block x sums list entries g, g+64, ... of
// column 16x + c (64 B coalesced row segments, 8 loads in flight) and the 64 row groups combine through LDS.
// The last block folds the three scalar heads.  Deterministic (fixed order).  With a sharp softmax the list
// holds a handful of rows and the kernel is launch-latency only.
__global__ __launch_bounds__(SUM_BLOCK) void summarize_kernel(const float* __restrict__ partials,
                                                          const float* __restrict__ heads,
                                                          const unsigned* __restrict__ min_key, int nblocks,
                                                          int colsp, int row, float* __restrict__ summary,
                                                          float* __restrict__ summary_copy,
                                                          int* __restrict__ nlive_out, P2pCtx p2p) {
    constexpr int NG = SUM_BLOCK / SUM_COLS;
    __shared__ float s_part[NG][SUM_COLS + 1];
    __shared__ unsigned short s_list[REDUCE_MAX_BLOCKS];
    __shared__ int s_wcnt[REDUCE_MAX_BLOCKS / WAVE];
    const int nlive = compact_live_rows<SUM_BLOCK>(heads, nblocks, s_list, s_wcnt);
    const int c = threadIdx.x & (SUM_COLS - 1), g = threadIdx.x / SUM_COLS;
    const bool head_block = blockIdx.x == gridDim.x - 1;
    float a[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = 0.f;
    const int col = blockIdx.x * SUM_COLS + c;
    const bool active = head_block ? c < 3 : col < colsp;
    const float* base = head_block ? heads + c : partials + col;
    const int64_t ld = head_block ? 4 : colsp;
    if (active) {
        for (int k = g; k < nlive; k += 8 * NG) {  // 8 independent loads in flight per thread
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int kk = k + q * NG;
                if (kk < nlive) a[q] += base[(int64_t)s_list[kk] * ld];
            }
        }
    }
    s_part[g][c] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    if (threadIdx.x < SUM_COLS) {
        float v = 0.f;
        for (int q = 0; q < NG; ++q) v += s_part[q][threadIdx.x];
        int dst = -1;
        if (!head_block) {
            const int cc = blockIdx.x * SUM_COLS + threadIdx.x;
            if (cc < row) dst = MPPI_SUMMARY_HEAD + cc;
        } else {
            if (threadIdx.x < 3) dst = 1 + threadIdx.x;
            if (threadIdx.x == 3) {
                dst = 0;
                v = key_to_float(*min_key);
                if (nlive_out) *nlive_out = nlive;
            }
        }
        if (dst >= 0) {
            summary[dst] = v;
            if (summary_copy) summary_copy[dst] = v;
            if (p2p.seq) {  // cells are self-contained: every block hands its own columns to the peers right away
                const size_t slot = ((size_t)(p2p.seq & 1u) * p2p.world + p2p.rank) * p2p.lenp + dst;
                const unsigned long long cell = cell_pack(p2p.seq, v);
                for (int w = 0; w < p2p.world; ++w) cell_store<__HIP_MEMORY_SCOPE_SYSTEM>(p2p.peers[w] + slot, cell);
            }
        }
    }
}

// mppi_finalize folds the partial rows itself while the reductions publish at most this many (sparse softmax);
// beyond it the multi-block summarize_kernel is cheaper than one block walking the rows.
static constexpr int FOLD_IN_FINALIZE_MAX_ROWS = 64;

// Short rows fold inside finalize_kernel (sparse softmax: no summarize launch); rows whose group sums do not fit the
// 64 KiB of LDS always take summarize_kernel.  A static property of the handle: the choice never depends on timing.
static bool fold_fits(mppi_handle_t h) {
    return FinalizeLds::floats(h->d.T, h->d.row, h->dc, 1, 255 /* widest filter */, true) * sizeof(float) <= 64 * 1024;
}

// grid of the layout conversions (inject_kernel, export_kernel): one block per tile and CONV_COLS columns of the row
static dim3 conv_grid(mppi_handle_t h) { return dim3((unsigned)h->d.tiles, (unsigned)((h->d.row + CONV_COLS - 1) / CONV_COLS)); }

// (`tm`: the stage the launch belongs to, or an untimed one)
static int materialize_tiles(mppi_handle_t h, StageTimer& tm) {
    const unsigned grid = (unsigned)((h->d.tiles + 3) / 4);
    if (!h->limits_set) return fail(h, MPPI_E_STATE, "dim_control > 4: call mppi_set_control_limits first");
    if (h->color.on) { if (int rc = sample_colored(h, tm)) return rc; }  // the filtered draw (always through the per-column tables)
    else if (h->wide || h->cov.on) tm.launch(sample_kernel<true>, dim3(grid), dim3(BLOCK), 0, h->core.noise, h->d, h->core.gen, (const float*)sigma_table(h));
    else tm.launch(sample_kernel<false>, dim3(grid), dim3(BLOCK), 0, h->core.noise, h->d, h->core.gen, (const float*)nullptr);
    HIP_TRY(h, hipGetLastError());
    h->core.tiles_valid = true;
    return MPPI_OK;
}

// the tiles must hold the current noise for the layout/gather entry points
int need_tiles(mppi_handle_t h, hipStream_t s) {
    if (h->core.tiles_valid) return MPPI_OK;
    StageTimer untimed(h, -1, s);
    return materialize_tiles(h, untimed);
}

// lambda argument of the reduce / finalize entry points -> (launch constant, device pointer or null)
int resolve_lambda(mppi_handle_t h, float lambda, const float** lam_dev) {
    *lam_dev = nullptr;
    if (lambda == MPPI_LAMBDA_DEVICE) {
        if (!h->search.lambda_dev_valid) return fail(h, MPPI_E_STATE, "MPPI_LAMBDA_DEVICE: no temperature on the device (run a device-resident rule or mppi_mpo_reset first)");
        *lam_dev = h->search.lambda_dev;
        return MPPI_OK;
    }
    if (!(lambda > 0.0f)) return fail(h, MPPI_E_INVALID, "lambda must be > 0");
    return MPPI_OK;
}

// Launch arguments of the control-cost term for `lambda` (> 0, MPPI_LAMBDA_DEVICE, or anything else: no temperature).  A
// device-resident rule that has not left a temperature yet gives the term a zero factor (the warm start of a first solve
// is zero anyway; the reference would multiply by the rule's name there).
static ActionCostArgs action_cost_args(mppi_handle_t h, float lambda) {
    ActionCostArgs a{};
    a.sigtab = (h->wide || h->cov.on) ? sigma_table(h) : nullptr;
    a.weight = h->ac.weight;
    if (lambda == MPPI_LAMBDA_DEVICE) a.lambda_dev = h->search.lambda_dev_valid ? h->search.lambda_dev.p : nullptr;
    else if (lambda > 0.0f) a.lambda = lambda;
    return a;
}

// A pending state sequence is about to be completed on `s`: if that is not the stream its finalize_kernel ran on, order `s`
// behind everything enqueued there so far (an event recorded NOW on the producing stream sits after finalize's write of b1).
static int order_behind_pending(mppi_handle_t h, hipStream_t s) {
    if (s == h->lazy.pending_stream) return MPPI_OK;
    if (!h->lazy.ev.e) HIP_TRY(h, hipEventCreateWithFlags(&h->lazy.ev.e, hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(h->lazy.ev.e, h->lazy.pending_stream));
    HIP_TRY(h, hipStreamWaitEvent(s, h->lazy.ev.e, 0));
    return MPPI_OK;
}

// The pending batch-1 rollout as its own one-wave kernel on `s` (same code and bits as the in-kernel rollout).  The pending
// mark is cleared only once the launch went through.
int flush_state_seq(mppi_handle_t h, hipStream_t s) {
    if (!h->lazy.pending_out) return MPPI_OK;
    float* out = h->lazy.pending_out;
    if (int rc = order_behind_pending(h, s)) return rc;
    const size_t sh1 = sizeof(float) * StateSeqLds::floats(h->d.row);
    StageTimer tm(h, 4, s);
#define CALL_STATE_SEQ(MODEL, FASTV)                                                                  \
    tm.launch(state_seq_kernel<MODEL, FASTV>, dim3(1), dim3(WAVE), sh1, (const float*)h->lazy.b1, h->d.row, h->d.T, out, h->model.ctx)
    MPPI_DISPATCH(h, CALL_STATE_SEQ);
#undef CALL_STATE_SEQ
    HIP_TRY(h, hipGetLastError());
    h->lazy.pending_out = nullptr;
    return MPPI_OK;
}

// ---- the single-launch solve (solve_fused_kernel)
static constexpr int64_t FUSED_AUTO_MAX_SAMPLES = 4096;          // fixed temperature / MPO
static constexpr int64_t FUSED_AUTO_MAX_SAMPLES_SEARCH = 16384;  // ESSPS / LBPS on the device
static bool fused_applies(mppi_handle_t h, float lambda) {
    if (!h->opt.fused_mode || h->cfg.model == MPPI_MODEL_GENERIC || h->opt.mapping != 0) return false;
    if (h->ac.on) return false;  // the control-cost term lives in the multi-kernel rollout only (like the covariance adaptation)
    if (h->part.P > 0) return false;  // ... and so does the rollout from a set of start states (mppi_set_particles)
    // measured (profiles/r03_experiments.md, r03_visitD_fused_crossover.txt): a cell round trip costs about as much as a
    // kernel boundary, so the single launch wins where it replaces more kernel boundaries than it needs round trips — with
    // a fixed temperature up to a few thousand samples (27 vs 32 us for racing at N = 1024, 29 vs 32 at 4096, 33 vs 32 at
    // 8192), under a temperature search further (nav2d ESSPS 32 vs 47 us at N = 1024, 48 vs 52 at 16 384, 51 vs 52 at 32 768)
    const bool search = lambda == MPPI_LAMBDA_DEVICE && (h->search.auto_rule == MPPI_AUTO_ESSPS || h->search.auto_rule == MPPI_AUTO_LBPS);
    // (the single launch searches LBPS on 32-temperature grids; the reference's Brent search is a kernel of its own)
    if (lambda == MPPI_LAMBDA_DEVICE && h->search.auto_rule == MPPI_AUTO_LBPS && !h->opt.lbps_grid) return false;
    if (h->opt.fused_mode == 1 && h->d.N > (search ? FUSED_AUTO_MAX_SAMPLES_SEARCH : FUSED_AUTO_MAX_SAMPLES)) return false;
    if (!regen_noise(h)) return false;                                                // the noise is regenerated in registers
    if (h->xchg.p2p_enabled || h->xchg.comm_enabled) return false;                      // sharded solves exchange between devices
    if (h->d.row > FUSED_MAX_ROW) return false;
    if (h->d.N > (int64_t)FUSED_BLOCK * std::min(FUSED_MAX_BLOCKS, h->cu_count)) return false;  // every block must be resident at once
    if (h->fused.error.get()) return false;                                   // a poll timed out once: stay on the multi-kernel path
    if (lambda == MPPI_LAMBDA_DEVICE && h->search.auto_rule == MPPI_AUTO_MPO && !h->search.lambda_dev_valid) return false;
    if (h->timers.mode == 1) return false;                                         // per-stage timing brackets the separate kernels
    return check_ready(h) == MPPI_OK;
}

static int solve_fused(mppi_handle_t h, float lambda, float* action_out, float* state_out, float* stats_out, hipStream_t s,
                       bool* declined) {
    *declined = false;
    if (!h->fused.cells) {  // first use: set-up path (blocking)
        HIP_TRY(h, h->fused.cells.alloc_set((size_t)FX_PHASES * FUSED_MAX_BLOCKS * FX_CELLS, 0));
        HIP_TRY(h, h->fused.grid0.alloc(STATS_L));
        HIP_TRY(h, h->fused.error.alloc(64, true));
        HIP_TRY(h, hipDeviceSynchronize());
    }
    const bool dev = lambda == MPPI_LAMBDA_DEVICE;
    int rule = FUSED_RULE_NONE;
    if (dev && h->search.auto_rule == MPPI_AUTO_ESSPS) rule = FUSED_RULE_ESSPS;
    if (dev && h->search.auto_rule == MPPI_AUTO_LBPS) rule = FUSED_RULE_LBPS;
    if (rule == FUSED_RULE_ESSPS)
        if (int rc = essps_prepare(h, h->search.auto_lo, h->search.auto_hi)) return rc;
    if (rule == FUSED_RULE_LBPS && (h->fused.grid0_lo != h->search.auto_lo || h->fused.grid0_hi != h->search.auto_hi)) {  // set-up path, blocking
        double g0[STATS_L];
        mppi::host::essps_make_grid<STATS_L>(h->search.auto_lo, h->search.auto_hi, g0);
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, hipMemcpy(h->fused.grid0, g0, sizeof(g0), hipMemcpyHostToDevice));
        h->fused.grid0_lo = h->search.auto_lo; h->fused.grid0_hi = h->search.auto_hi;
    }
    if (!dev && !(lambda > 0.0f)) return fail(h, MPPI_E_INVALID, "lambda must be > 0");
    const auto mk = h->min_key.begin_rollout();
    next_tag(h->seq.fused);
    FusedArgs A{};
    A.mean = h->core.mean; A.x0 = h->core.x0_cur; A.costs = h->core.costs;
    A.min_key = mk.accumulate; A.next_min_key = mk.reset_next;
    A.mean_used = h->core.mean_used; A.x0_used = h->core.x0_used;
    A.rule = rule; A.rule_param = h->search.auto_param; A.lam_min = h->search.auto_lo; A.lam_max = h->search.auto_hi;
    A.lambda_arg = dev ? -1.0f : lambda;
    A.lambda_dev = h->search.lambda_dev; A.lambda_host = &h->search.mirror.dev->lam_next;
    A.grid0 = rule == FUSED_RULE_ESSPS ? h->search.essps_dev.p->grid0 : h->fused.grid0;
    A.lams0 = h->search.lams_dev + STATS_L;
    A.essps = h->search.essps_dev; A.range = h->search.essps_range;
    A.mean_store = h->core.mean; A.action_out = action_out; A.state_out = state_out; A.stats_out = stats_out;
    A.stats_keep = h->reduce.solve_stats; A.summary_out = h->reduce.summary;
    const SgFilter sg{h->reduce.sg_coeffs, h->reduce.sg_history, h->reduce.sg_window};
    const FusedCtx fx{h->fused.cells, h->fused.error.dev, h->seq.fused, h->opt.fused_timeout_ticks};
    // G = min(#CUs, ceil(N / 64)) blocks, each owning spb (a multiple of 64, <= 512) consecutive trajectories: ONE wave
    // of rollouts per block as long as there are CUs left (the rest of its 512 threads share the block's reductions and
    // the regeneration of its weighted noise rows, which a block of 256 trajectories spends ~5 us on)
    const int64_t gmax = std::min(FUSED_MAX_BLOCKS, h->cu_count);
    unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(gmax, (h->d.N + 63) / 64));
    // up to FUSED_AUTO_MAX_SAMPLES trajectories: at most FUSED_SMALL_BLOCKS blocks, which then need neither the hop for the
    // global minimum nor the broadcast of the temperature (solve_fused_kernel: `small`)
    if (h->d.N <= FUSED_AUTO_MAX_SAMPLES) grid = std::min<unsigned>(grid, (unsigned)FUSED_SMALL_BLOCKS);
    A.spb = (int)(((h->d.N + grid - 1) / grid + 63) / 64 * 64);
    grid = (unsigned)((h->d.N + A.spb - 1) / A.spb);  // (no block without trajectories)
    h->fused.last_blocks = (int)grid; h->fused.last_spb = A.spb;  // (mppi_fused_geometry; cleared by mppi_solve if the launch is declined)
#define CALL_FUSED(MODEL, FASTV)                                                                      \
    do {                                                                                              \
        const size_t shmem = sizeof(float) * FusedLds::floats(h->d.R, h->d.T, h->d.row, h->dc, ModelT<MODEL, FASTV>::KROW, sg.window); \
        /* the blocks synchronise through cells in HBM: every one of them must be resident at once.  Checked against the   \
           kernel's own occupancy (cached per (math level, LDS size)); what OTHER work holds of the GPU at run time is what  \
           the polls' time-out is for */                                                                                   \
        const bool track = mlp_track(MODEL) && mlp_tracking(h->model.ctx);  /* (the learned models: mppi_models.hpp) */          \
        const uint64_t okey = ((uint64_t)(FASTV + 1) << 48) | ((uint64_t)track << 47) | (uint64_t)shmem;                  \
        const auto kern = track ? solve_fused_kernel<MODEL, FASTV, mlp_track(MODEL)> : solve_fused_kernel<MODEL, FASTV, false>; \
        if (h->fused.occ_key != okey) {                                                                                    \
            int nb = 0;                                                                                                    \
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, FUSED_BLOCK, shmem) != hipSuccess) nb = 0;          \
            h->fused.occ_key = okey; h->fused.occ_blocks = nb;                                                             \
        }                                                                                                                  \
        if ((int64_t)grid > (int64_t)h->fused.occ_blocks * h->cu_count) { *declined = true; break; }                       \
        StageTimer tm(h, 1, s);  /* (after the occupancy check: a declined launch leaves no empty event pair behind) */    \
        tm.launch(kern, dim3(grid), dim3(FUSED_BLOCK), shmem, A, h->d, h->core.gen, h->model.ctx, sg, fx);  \
    } while (0)
    MPPI_DISPATCH(h, CALL_FUSED);
#undef CALL_FUSED
    if (*declined) {  // (undo the bookkeeping of a solve that did not start: the multi-kernel path takes it from here)
        h->min_key.cancel_rollout();
        --h->seq.fused;
        return MPPI_OK;
    }
    HIP_TRY(h, hipGetLastError());
    if (rule != FUSED_RULE_NONE) h->search.lambda_dev_valid = true;
    // (the single launch rolls the solution out itself; a state sequence still pending from an earlier multi-kernel solve
    // was completed by mppi_solve before it got here)
    h->reduce.last_reduce_blocks = 0;   // no partial rows of a separate reduction exist for this solve
    h->reduce.summary_valid = true;     // ... but its summary does (h->reduce.summary)
    return MPPI_OK;
}

}  // namespace mppi

extern "C" {

int mppi_sample(mppi_handle_t h, uint32_t solve_idx, void* stream) {
    if (!h) return MPPI_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    h->core.gen.solve_idx = solve_idx;
    h->core.injected = false;
    h->core.tiles_valid = false;
    // (`injected` was cleared two lines up, so this is the handle's standing answer)
    if (regen_noise(h)) return MPPI_OK;  // consumers regenerate eps(seed, solve, i, t, k) in registers
    StageTimer tm(h, 0, s);
    return materialize_tiles(h, tm);
}

int mppi_inject_noise(mppi_handle_t h, const float* eps_dev, void* stream) {
    if (!h || !eps_dev) return fail(h, MPPI_E_INVALID, "null");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(inject_kernel, conv_grid(h), dim3(BLOCK), 0, s, eps_dev, h->core.noise, h->d);
    HIP_TRY(h, hipGetLastError());
    h->core.injected = true;
    h->core.tiles_valid = true;
    return MPPI_OK;
}

int mppi_export_noise(mppi_handle_t h, float* eps_out, float* act_out, void* stream) {
    if (!h) return MPPI_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = need_tiles(h, s)) return rc;
    hipLaunchKernelGGL(export_kernel, conv_grid(h), dim3(BLOCK), 0, s, h->core.noise, h->core.mean, eps_out, act_out, h->d,
                       h->wide ? h->core.coltab : (const float*)nullptr);
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

int mppi_rollout_cost(mppi_handle_t h, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (int rc = check_ready(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (h->ac.on && h->opt.mapping == 1) return fail(h, MPPI_E_INVALID, "the control-cost term is not available with mapping = 1");
    if (h->part.P > 0) return rollout_particles(h, s);  // risk-aware solves: every sample from every particle, then the fold
    if (h->opt.mapping == 1) {  // comparison variant: one wavefront per trajectory, reference-layout noise
        if (int rc = flush_state_seq(h, s)) return rc;
        if (!h->core.noise_std) HIP_TRY(h, h->core.noise_std.alloc((size_t)h->d.N * h->d.row));
        if (int rc = need_tiles(h, s)) return rc;
        hipLaunchKernelGGL(export_kernel, conv_grid(h), dim3(BLOCK), 0, s, h->core.noise, h->core.mean, h->core.noise_std, (float*)nullptr, h->d,
                           (const float*)nullptr);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->core.mean_used, h->core.mean, sizeof(float) * (size_t)h->d.row, hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(h->core.x0_used, h->core.x0_cur, sizeof(float) * (size_t)h->ds, hipMemcpyDeviceToDevice, s));
        StageTimer tmw(h, 1, s);
        const auto mkw = h->min_key.begin_rollout();
        const unsigned wgrid = (unsigned)std::min<int64_t>((h->d.N + 3) / 4, 256 * 8 * 4);
#define CALL_WAVE(MODEL, FASTV)                                                                       \
        do {                                                                                          \
            const size_t shw = sizeof(float) * WaveRolloutLds::floats(h->d.R, h->d.T, ModelT<MODEL, FASTV>::DS);          \
            tmw.launch(mlp_track(MODEL) && mlp_tracking(h->model.ctx) ? rollout_cost_wave_kernel<MODEL, FASTV, mlp_track(MODEL)>      \
                                                                      : rollout_cost_wave_kernel<MODEL, FASTV, false>, dim3(wgrid), dim3(BLOCK), shw, h->core.noise_std,      \
                       h->core.mean, h->core.x0_cur, h->core.costs, mkw.accumulate, mkw.reset_next, h->d, h->model.ctx); \
        } while (0)
        MPPI_DISPATCH(h, CALL_WAVE);
#undef CALL_WAVE
        HIP_TRY(h, hipGetLastError());
        return MPPI_OK;
    }
    StageTimer tm(h, 1, s, true);  // (this stage's one kernel stamps its own time)
    const bool gen = regen_noise(h);  // (check_ready has refused generic handles, the only wide ones)
    if (!gen && !h->core.tiles_valid) return fail(h, MPPI_E_STATE, "no noise: call mppi_sample or mppi_inject_noise first");
    const auto mk = h->min_key.begin_rollout();
    // a state sequence still pending from the previous solve (option "lazy_state_seq") rides in one extra block of this
    // launch: its T dependent steps hide behind the N-sample rollout instead of extending the previous solve's tail
    float* ride = h->lazy.pending_out;
    if (ride) { if (int rc = order_behind_pending(h, s)) return rc; }
    const unsigned grid = (unsigned)((h->d.tiles + 3) / 4) + (ride ? 1u : 0u);
    unsigned long long* stamps = tm.take_stamps();
    const bool term = h->ac.on;  // the control-cost term: its own instantiations, 4R more floats of LDS for g
    const ActionCostArgs aca = action_cost_args(h, h->ac.lambda);
#define ROLLOUT_ARGS                                                                                  \
    h->core.noise, h->core.mean, h->core.x0_cur, h->core.costs, mk.accumulate, mk.reset_next, h->core.mean_used, h->core.x0_used, \
    h->d, h->core.gen, h->model.ctx, (const float*)h->lazy.b1, ride, stamps
#define CALL_ROLLOUT(MODEL, FASTV)                                                                    \
    do {                                                                                              \
        const size_t shmem = sizeof(float) * RolloutLds::floats(h->d.R, h->d.T, h->d.row, ModelT<MODEL, FASTV>::KROW, term); \
        constexpr bool UCV = FASTV != 0;  /* the FAST kernels exist in the u_in_bounds form only (see use_fast) */ \
        constexpr bool TRK = mlp_track(MODEL);  /* (the learned models' instantiations with the tracking cost: mppi_models.hpp) */ \
        if (TRK && mlp_tracking(h->model.ctx)) {                                                      \
            if (term)                                                                                 \
                tm.launch(gen ? rollout_action_cost_kernel<MODEL, FASTV, true, UCV, TRK> : rollout_action_cost_kernel<MODEL, FASTV, false, UCV, TRK>, \
                          dim3(grid), dim3(BLOCK), shmem, ROLLOUT_ARGS, aca);                         \
            else                                                                                      \
                tm.launch(gen ? rollout_cost_kernel<MODEL, FASTV, true, UCV, TRK> : rollout_cost_kernel<MODEL, FASTV, false, UCV, TRK>, \
                          dim3(grid), dim3(BLOCK), shmem, ROLLOUT_ARGS);                              \
        } else if (term)                                                                              \
            tm.launch(gen ? rollout_action_cost_kernel<MODEL, FASTV, true, UCV> : rollout_action_cost_kernel<MODEL, FASTV, false, UCV>, \
                      dim3(grid), dim3(BLOCK), shmem, ROLLOUT_ARGS, aca);                             \
        else                                                                                          \
            tm.launch(gen ? rollout_cost_kernel<MODEL, FASTV, true, UCV> : rollout_cost_kernel<MODEL, FASTV, false, UCV>, \
                      dim3(grid), dim3(BLOCK), shmem, ROLLOUT_ARGS);                                  \
    } while (0)
    MPPI_DISPATCH(h, CALL_ROLLOUT);
#undef CALL_ROLLOUT
#undef ROLLOUT_ARGS
    HIP_TRY(h, hipGetLastError());
    if (ride) h->lazy.pending_out = nullptr;  // (cleared only once the launch that carries it went through)
    return MPPI_OK;
}

#ifdef MPPI_ROLLOUT_TRACE
// (experiments only) the [4 * blocks][6] device buffer that the next rollout launches stamp their timeline into; null: none
extern "C" int mppi_debug_rollout_trace(void* rows_dev) {
    unsigned long long* p = (unsigned long long*)rows_dev;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_rollout_trace), &p, sizeof(p)) == hipSuccess ? MPPI_OK : MPPI_E_HIP;
}
#endif

int mppi_get_costs(mppi_handle_t h, float* dst, int on_device, void* stream) {
    if (!h || !dst) return fail(h, MPPI_E_INVALID, "null");
    return copy_small(h, dst, h->core.costs, sizeof(float) * (size_t)h->d.N, on_device != 0, true, (hipStream_t)stream);
}

__global__ void min_cost_kernel(const float* __restrict__ costs, int64_t N, unsigned* __restrict__ min_key) {
    float m = INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
        m = fminf(m, costs[i]);
    m = wave_min(m);
    if ((threadIdx.x & 63) == 0 && m < INFINITY) atomicMin(min_key, float_to_key(m));
}

// The costs were replaced by something other than a rollout: the current minimum key is computed from them again.
static int refresh_min_key(mppi_handle_t h, hipStream_t s) {
    HIP_TRY(h, hipMemsetAsync(h->min_key.cur_rw(), 0xFF, sizeof(unsigned), s));
    const unsigned grid = (unsigned)std::min<int64_t>((h->d.N + BLOCK - 1) / BLOCK, 1024);
    hipLaunchKernelGGL(min_cost_kernel, dim3(grid), dim3(BLOCK), 0, s, h->core.costs, h->d.N, h->min_key.cur_rw());
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

int mppi_set_costs(mppi_handle_t h, const float* src, int on_device, void* stream) {
    if (!h || !src) return fail(h, MPPI_E_INVALID, "null");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = copy_small(h, h->core.costs, src, sizeof(float) * (size_t)h->d.N, true, on_device != 0, s)) return rc;
    return refresh_min_key(h, s);
}

// costs[i] += kappa * A_i from the noise tiles: the control-cost term as a pass of its own (mppi_add_action_cost).  One
// lane per sample, the groups of its row in order — the same operations in the same order as the rollout kernel's lanes.
__global__ __launch_bounds__(BLOCK) void action_cost_kernel(const float4* __restrict__ noise, const float* __restrict__ mean,
                                                            float* __restrict__ costs, Dims d,
                                                            const float* __restrict__ coltab /* wide rows, else null */,
                                                            ActionCostArgs ac) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= d.N) return;
    const int64_t tile = i >> 6;
    const int lane = (int)(i & 63);
    const bool inherit = (d.sample_offset + i) < d.inherit_count;
    const int dc = d.dc;
    float A = 0.0f;
    for (int r = 0; r < d.R; ++r) {
        const float4 e4 = noise[(tile * d.R + r) * 64 + lane];
        const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = 4 * r + j;
            if (f >= d.row) break;
            const int k = f % dc;
            const float m = mean[f];
            const float sg = ac.sigtab ? ac.sigtab[f] : d.sigma[k];
            float lo, hi;
            if (coltab) { lo = coltab[4 * d.R + f]; hi = coltab[8 * d.R + f]; }
            else { lo = d.u_min[k]; hi = d.u_max[k]; }
            const float g = action_cost_g(m, action_cost_inv(f / dc, sg));
            const float u = clampf((inherit ? m : 0.0f) + ev[j], lo, hi);
            A = action_cost_accumulate(A, g, u);
        }
    }
    const float kappa = action_cost_kappa(ac.weight, ac.lambda_dev ? *ac.lambda_dev : ac.lambda);
    costs[i] = action_cost_total(costs[i], kappa, A);
}

int mppi_set_action_cost(mppi_handle_t h, int enable, float weight) {
    if (!h) return MPPI_E_INVALID;
    if (!(weight >= 0.0f) || !std::isfinite(weight)) return fail(h, MPPI_E_INVALID, "control-cost term: the weight must be finite and >= 0");
    if (enable && h->opt.mapping == 1) return fail(h, MPPI_E_INVALID, "the control-cost term is not available with mapping = 1");
    if (enable)
        for (int k = 0; k < std::min(h->dc, (int)MPPI_MAX_DIM_CONTROL); ++k)
            if (!(h->d.sigma[k] > 0.0f)) return fail(h, MPPI_E_INVALID, "control-cost term: every sigma must be > 0");
    if (int rc = settle_state_seq(h)) return rc;  // (a pending state sequence rides in the rollout launch of ITS setting)
    h->ac.on = enable != 0;
    h->ac.weight = weight;
    return MPPI_OK;
}

// the temperature argument of the control-cost entry points
static int check_action_cost_lambda(mppi_handle_t h, float lambda) {
    if (lambda != MPPI_LAMBDA_DEVICE && (!(lambda >= 0.0f) || !std::isfinite(lambda)))
        return fail(h, MPPI_E_INVALID, "control-cost term: lambda must be >= 0 or MPPI_LAMBDA_DEVICE");
    return MPPI_OK;
}

int mppi_set_action_cost_lambda(mppi_handle_t h, float lambda) {
    if (!h) return MPPI_E_INVALID;
    if (int rc = check_action_cost_lambda(h, lambda)) return rc;
    h->ac.lambda = lambda;
    return MPPI_OK;
}

int mppi_add_action_cost(mppi_handle_t h, float lambda, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (int rc = check_action_cost_lambda(h, lambda)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = need_tiles(h, s)) return rc;
    const unsigned agrid = (unsigned)((h->d.N + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(action_cost_kernel, dim3(agrid), dim3(BLOCK), 0, s, h->core.noise, h->core.mean, h->core.costs, h->d,
                       h->wide ? (const float*)h->core.coltab : (const float*)nullptr, action_cost_args(h, lambda));
    HIP_TRY(h, hipGetLastError());
    return refresh_min_key(h, s);
}

int mppi_weights_reduce(mppi_handle_t h, float lambda, float* summary_out_dev, void* stream) {
    if (!h) return MPPI_E_INVALID;
    const float* lam_dev = nullptr;
    if (int rc = resolve_lambda(h, lambda, &lam_dev)) return rc;
    hipStream_t s = (hipStream_t)stream;
    // Which launches the stage makes is known up front.  The published partial rows are folded into the shard summary by
    // summarize_kernel when sharded use needs the summary before the collective; otherwise mppi_finalize folds the rows
    // itself when the previous solves published few of them (*live_hint, written by finalize_kernel to mapped host memory
    // and read here without synchronising: it only steers this choice: both folds use the same summation tree, so the
    // summary is bit-identical either way).
    const bool many_rows = h->opt.fold_mode == 0 ? *(volatile int*)h->reduce.live_hint.host > FOLD_IN_FINALIZE_MAX_ROWS : h->opt.fold_mode == 2;
    const bool comm = h->xchg.comm_enabled && !h->xchg.p2p_enabled;
    // (covariance adaptation: the step between this call and mppi_finalize reads the summary)
    const bool summarize = summary_out_dev || h->xchg.p2p_enabled || comm || !fold_fits(h) || many_rows || h->cov.on;
    StageTimer tm(h, 2, s);
    tm.left = comm ? 0 : summarize ? 2 : 1;  // (the all-gather ends the stage: its stop event is recorded behind it)
    // one wave per tile up to reduce_blocks blocks (dense weights need the parallelism; with sparse
    // weights most waves only run the phase-A check)
    int64_t blocks = std::min<int64_t>(h->opt.reduce_blocks, (h->d.tiles + 3) / 4);
    blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, REDUCE_MAX_BLOCKS));
    h->reduce.last_reduce_blocks = (int)blocks;
    const dim3 grid((unsigned)blocks, (unsigned)h->reduce.nchunks);
    const bool gen = regen_noise(h);
    if (!gen && !h->core.tiles_valid) return fail(h, MPPI_E_STATE, "no noise: call mppi_sample or mppi_inject_noise first");
    const unsigned* mk = h->min_key.cur();
#define CALL_REDUCE(GPWV, GENV, WIDEV, CHAINSV, REMV)                                                 \
    tm.launch(weights_reduce_kernel<GPWV, GENV, WIDEV, CHAINSV, REMV>, grid, dim3(BLOCK), 0, h->core.noise, h->core.mean, h->core.costs, mk, \
              h->reduce.partials, h->reduce.heads, h->d, h->core.gen, lambda, lam_dev, (const float*)h->core.coltab)
    // regenerated noise: four chains per basic block while a SIMD holds one or two reduction waves, two beyond (see the kernel)
    const bool chains4 = h->opt.reduce_chains == 4 || (h->opt.reduce_chains == 0 && blocks * (int64_t)h->reduce.nchunks <= 2 * (int64_t)h->cu_count);
    const bool rem = (h->d.R % 4) != 0;  // some chunk of the row leaves groups over (chunks hold 32 groups: R % 32 % 4)
    if (h->wide) CALL_REDUCE(8, false, true, 2, true);
    else if (gen && chains4 && rem) CALL_REDUCE(8, true, false, 4, true);
    else if (gen && chains4) CALL_REDUCE(8, true, false, 4, false);
    else if (gen && rem) CALL_REDUCE(8, true, false, 2, true);
    else if (gen) CALL_REDUCE(8, true, false, 2, false);
    else if (rem) CALL_REDUCE(8, false, false, 2, true);
    else CALL_REDUCE(8, false, false, 2, false);
#undef CALL_REDUCE
    HIP_TRY(h, hipGetLastError());
    h->reduce.summary_valid = false;
    P2pCtx p2p{};
    if (h->xchg.p2p_enabled) {  // summarize_kernel also hands the summary to every peer (and to this rank's own slot)
        next_tag(h->seq.p2p);
        p2p = p2p_ctx(h);
    }
    if (comm && summary_out_dev) return fail(h, MPPI_E_INVALID, "exchange_comm: the library gathers the summaries itself (pass NULL)");
    if (summarize) {
        const unsigned sgrid = (unsigned)((h->reduce.colsp + SUM_COLS - 1) / SUM_COLS + 1);
        tm.launch(summarize_kernel, dim3(sgrid), dim3(SUM_BLOCK), 0, h->reduce.partials, h->reduce.heads, mk, (int)blocks,
                  h->reduce.colsp, h->d.row, h->reduce.summary, comm ? h->xchg.comm_send : summary_out_dev, h->reduce.live_hint.dev, p2p);
        HIP_TRY(h, hipGetLastError());
        h->reduce.summary_valid = true;
    }
    if (comm)  // the solve's only exchange: 4 + T*dc floats per rank, on the solve's own stream
        RCCL_TRY(h, rccl().all_gather(h->xchg.comm_send, h->xchg.comm_recv, (size_t)(MPPI_SUMMARY_HEAD + h->d.row), ncclFloat, h->xchg.comm, s));
    h->cov.ready = h->cov.on;
    return MPPI_OK;
}

int mppi_finalize(mppi_handle_t h, const float* summaries_dev, int num_shards, float lambda, int store_mean,
                  float* action_out, float* state_out, float* stats_out, void* stream) {
    if (!h || num_shards < 1) return fail(h, MPPI_E_INVALID, "bad finalize arguments");
    const float* lam_dev = nullptr;
    if (int rc = resolve_lambda(h, lambda, &lam_dev)) return rc;
    const bool generic = h->cfg.model == MPPI_MODEL_GENERIC;
    if (generic && state_out) return fail(h, MPPI_E_INVALID, "generic model: roll the action out with the host dynamics");
    if (!generic) { if (int rc = check_ready(h)) return rc; }
    hipStream_t s = (hipStream_t)stream;
    P2pCtx p2p{};  // seq == 0: off
    if (!summaries_dev) {  // this handle's own reduction (mppi_weights_reduce)
        if (h->reduce.last_reduce_blocks < 1) return fail(h, MPPI_E_STATE, "mppi_finalize before mppi_weights_reduce");
        if (h->xchg.p2p_enabled) {
            p2p = p2p_ctx(h);  // all shards' summaries of this solve, through the exchange buffer
            num_shards = h->xchg.p2p_world;
        } else if (h->xchg.comm_enabled) {
            summaries_dev = h->xchg.comm_recv;  // gathered by mppi_weights_reduce
            num_shards = h->xchg.comm_world;
        } else {
            if (h->reduce.summary_valid) summaries_dev = h->reduce.summary;  // else the kernel folds the partial rows itself
            num_shards = 1;
        }
    }
    // the filter replaces the stored warm start, so it only runs when this call stores it (mppi.py:441-452)
    const SgFilter sg{h->reduce.sg_coeffs, h->reduce.sg_history, (store_mean && h->reduce.sg_window > 0) ? h->reduce.sg_window : 0};
    const bool fold_here = !summaries_dev && !p2p.seq;  // the kernel folds the partial rows itself
    const size_t shmem = FinalizeLds::floats(h->d.T, h->d.row, h->dc, p2p.seq ? p2p.world : 1, sg.window, fold_here) * sizeof(float);
    if (shmem > 64 * 1024) return fail(h, MPPI_E_INVALID, "finalize: horizon too long for the exchange / filter staging");
    const unsigned* mk = h->min_key.cur();
    // Option "lazy_state_seq": the batch-1 rollout leaves this kernel (and the solve's critical path).  The kernel writes the
    // rollout's inputs to h->lazy.b1; the rollout itself rides in the next mppi_rollout_cost launch on this stream, or is
    // launched by mppi_join_state_seq when somebody reads the state sequence first.
    const bool defer = h->lazy.on && state_out && !generic && h->opt.mapping == 0;
    if (h->lazy.pending_out) { if (int rc = flush_state_seq(h, s)) return rc; }  // (an older one nobody picked up)
    {
        StageTimer tm(h, 3, s);
#define CALL_FINALIZE(MODEL, FASTV)                                                                   \
    tm.launch(finalize_kernel<MODEL, FASTV>, dim3(1), dim3(FIN_BLOCK), shmem, summaries_dev, num_shards,               \
                       h->reduce.partials, h->reduce.heads, mk, h->reduce.last_reduce_blocks, h->reduce.colsp, h->reduce.summary, h->reduce.live_hint.dev,  \
                       lambda, lam_dev, h->d.row, h->d.T, h->core.x0_cur, store_mean ? h->core.mean : (float*)nullptr, action_out,  \
                       defer ? (float*)nullptr : state_out, stats_out, h->reduce.solve_stats, sg, p2p, h->model.ctx,          \
                       defer ? h->lazy.b1 : (float*)nullptr, defer ? state_out : (float*)nullptr)
        MPPI_DISPATCH(h, CALL_FINALIZE);
#undef CALL_FINALIZE
    }
    HIP_TRY(h, hipGetLastError());
    h->cov.ready = false;  // (a stored warm start is no longer the mean this solve sampled around)
    ++h->lazy.finalize_serial;
    if (defer) { h->lazy.pending_out = state_out; h->lazy.pending_serial = h->lazy.finalize_serial; h->lazy.pending_stream = s; }
    return MPPI_OK;
}

// Complete the state sequence of the last mppi_finalize / mppi_solve on `stream` if its rollout is still pending (option
// "lazy_state_seq"); a no-op otherwise.  `serial` = 0, or the value mppi_state_seq_serial returned right after that solve:
// a reader of an OLDER solve's state sequence (already completed by a later rollout launch) then launches nothing.
int mppi_join_state_seq(mppi_handle_t h, uint32_t serial, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (!h->lazy.pending_out || (serial && serial != h->lazy.pending_serial)) return MPPI_OK;
    return flush_state_seq(h, (hipStream_t)stream);
}

// Serial number of the last mppi_finalize (for mppi_join_state_seq), and whether its state sequence is still pending.
int mppi_state_seq_serial(mppi_handle_t h, uint32_t* serial_out, int* pending_out) {
    if (!h) return MPPI_E_INVALID;
    if (serial_out) *serial_out = h->lazy.finalize_serial;
    if (pending_out) *pending_out = h->lazy.pending_out != nullptr && h->lazy.pending_serial == h->lazy.finalize_serial;
    return MPPI_OK;
}

// The temperature rule mppi_solve applies when it is called with lambda = MPPI_LAMBDA_DEVICE (mppi.py:183-210).
int mppi_set_auto_lambda(mppi_handle_t h, int rule, double param, double lam_min, double lam_max) {
    if (!h || rule < MPPI_AUTO_NONE || rule > MPPI_AUTO_MPO) return fail(h, MPPI_E_INVALID, "bad temperature rule");
    if ((rule == MPPI_AUTO_ESSPS || rule == MPPI_AUTO_LBPS) && (!(lam_min > 0.0) || !(lam_max > lam_min) || !(param > 0.0)))
        return fail(h, MPPI_E_INVALID, "bad temperature rule arguments");
    h->search.auto_rule = rule; h->search.auto_param = param; h->search.auto_lo = lam_min; h->search.auto_hi = lam_max;
    return MPPI_OK;
}

// MPPI.forward() for a native model in ONE call (mppi.py:223-460): bind the state, fix the noise identity, rollout +
// costs, the temperature (fixed, or the configured rule resident on the device), weights + reduction, finalize with the
// warm start stored.  Exactly the sequence of the individual entry points (same kernels, same results): one
// host -> library transition per solve for callers that need nothing in between.
int mppi_solve(mppi_handle_t h, const float* x0_dev, uint32_t solve_idx, float lambda, float* action_out_dev,
               float* state_seq_out_dev, float* stats_out_dev, void* stream) {
    if (!h) return MPPI_E_INVALID;
    const bool dev = lambda == MPPI_LAMBDA_DEVICE;
    if (dev && h->search.auto_rule == MPPI_AUTO_NONE)
        return fail(h, MPPI_E_STATE, "MPPI_LAMBDA_DEVICE: no temperature rule configured (mppi_set_auto_lambda)");
    if (x0_dev) h->core.x0_cur = x0_dev;  // (mppi_bind_state)
    if (h->ac.on) h->ac.lambda = lambda;  // the term's temperature is this solve's argument (mppi_set_action_cost_lambda)
    if (int rc = mppi_sample(h, solve_idx, stream)) return rc;
    if (fused_applies(h, lambda)) {
        if (int rc = flush_state_seq(h, (hipStream_t)stream)) return rc;  // (pending from an earlier multi-kernel solve)
        bool declined = false;
        if (int rc = solve_fused(h, lambda, action_out_dev, state_seq_out_dev, stats_out_dev, (hipStream_t)stream, &declined)) return rc;
        if (!declined) {
            if (h->search.auto_rule == MPPI_AUTO_MPO) return mppi_mpo_step_device(h, stream);
            return MPPI_OK;
        }
    }
    h->fused.last_blocks = h->fused.last_spb = 0;  // this solve is the multi-kernel path (mppi_fused_geometry)
    if (int rc = mppi_rollout_cost(h, stream)) return rc;
    if (dev && h->search.auto_rule == MPPI_AUTO_ESSPS) {
        if (int rc = mppi_essps_lambda_device(h, h->search.auto_param, h->search.auto_lo, h->search.auto_hi, stream)) return rc;
    } else if (dev && h->search.auto_rule == MPPI_AUTO_LBPS) {
        if (int rc = h->opt.lbps_grid ? mppi_lbps_lambda_device(h, h->search.auto_param, h->search.auto_lo, h->search.auto_hi, stream)
                                  : mppi_lbps_brent_device(h, h->search.auto_param, h->search.auto_lo, h->search.auto_hi, stream)) return rc;
    }
    if (int rc = mppi_weights_reduce(h, lambda, nullptr, stream)) return rc;
    if (h->cov.on) { if (int rc = mppi_update_covariance(h, lambda, stream)) return rc; }
    if (int rc = mppi_finalize(h, nullptr, 1, lambda, 1, action_out_dev, state_seq_out_dev, stats_out_dev, stream)) return rc;
    // MPO: the dual steps after every solve, whatever temperature this solve's weights were given (mppi.py:387-398)
    if (h->search.auto_rule == MPPI_AUTO_MPO) return mppi_mpo_step_device(h, stream);
    return MPPI_OK;
}

// Savitzky-Golay smoothing of the solution inside mppi_finalize (step 7, mppi.py:423-443): taps = first row of
// pinv(vander) computed by the caller (mppi.py:568-596), history = `_actions_history_for_sg`.
int mppi_set_sg_filter(mppi_handle_t h, const float* coeffs_host, int window, const float* history_host) {
    if (!h || window < 0) return fail(h, MPPI_E_INVALID, "bad sg filter arguments");
    if (window == 0) { h->reduce.sg_window = 0; return MPPI_OK; }
    if (!coeffs_host || window % 2 == 0 || window > 255) return fail(h, MPPI_E_INVALID, "sg window must be odd and <= 255");
    if (h->d.row > FIN_BLOCK) return fail(h, MPPI_E_INVALID, "sg filter on the device supports T*dim_control <= 1024");
    if (window / 2 > 2 * h->d.T - 1) return fail(h, MPPI_E_INVALID, "sg window too wide for the horizon");
    const size_t hist_floats = (size_t)std::max(h->d.T - 1, 1) * h->dc;
    if (!h->reduce.sg_coeffs) HIP_TRY(h, h->reduce.sg_coeffs.alloc(256));
    if (!h->reduce.sg_history) HIP_TRY(h, h->reduce.sg_history.alloc_set(hist_floats, 0));
    HIP_TRY(h, hipMemcpy(h->reduce.sg_coeffs, coeffs_host, sizeof(float) * (size_t)window, hipMemcpyHostToDevice));
    if (history_host)
        HIP_TRY(h, hipMemcpy(h->reduce.sg_history, history_host, sizeof(float) * (size_t)(h->d.T - 1) * h->dc, hipMemcpyHostToDevice));
    h->reduce.sg_window = window;
    return MPPI_OK;
}

int mppi_get_sg_history(mppi_handle_t h, float* history_host) {
    if (!h || !history_host) return fail(h, MPPI_E_INVALID, "null");
    if (!h->reduce.sg_history) return fail(h, MPPI_E_STATE, "sg filter not set");
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(history_host, h->reduce.sg_history, sizeof(float) * (size_t)(h->d.T - 1) * h->dc, hipMemcpyDeviceToHost));
    return MPPI_OK;
}

}  // extern "C"
