// mppi_handle.hpp — the handle behind include/mppi_hip.h and the host helpers the capi_*.hip units share.
// Host-only: no kernels.
//
// Mapping (CDNA4, wave64): one LANE per trajectory, one WAVEFRONT per tile of 64 trajectories.  The horizon recurrence
// is serial in t, so the 64 lanes of a wave advance 64 independent trajectories in lock-step; the noise is stored
// lane-major (see include/mppi_hip.h) so each wave-level load/store is one contiguous 1 KiB segment, no LDS transpose is
// needed on the hot path, and state stays in VGPRs for the whole horizon.  LDS is used only for the block-level
// reductions and for the [N][T][dc] <-> tile layout conversions (inject/export).
//
// Host units (C ABI), each including the kernel headers it launches from:
//   capi_handle.hip    create / destroy / clone, options, timing, mean and state
//   capi_model.hip     model parameters, maps, reference window, disc table, env.step (mppi_maps.hpp, mppi_env.hpp)
//   capi_solve.hip     the solve: sample, rollout, reduce, finalize, fused, mppi_solve (+ summarize_kernel)
//   capi_search.hip    softmax statistics, ESSPS / LBPS / Brent / MPO               (+ the non-template search kernels)
//   capi_topk.hip      queries after a solve                                         (mppi_topk.hpp)
//   capi_exchange.hip  RCCL loader, comm / p2p exchanges, time-out flags             (+ the p2p kernels)
//   capi_covariance.hip  covariance adaptation: settings, the per-step sigma table, the step after the weights (mppi_variance.hpp)
//   capi_colored.hip   temporally correlated noise: the setting, its per-column table, the filtered draws (mppi_sample.hpp)
//   capi_particles.hip risk-aware solves: the particle table, the risk measure, the rollout from every particle (each through
//                      a member of an MLP ensemble of its own, where a map says so) and the fold
//                      (mppi_particles.hpp: rollout_particles_kernel, particle_fold_kernel)
// Kernel headers, one per stage.  A kernel that is not a template is defined in the one unit that launches it.
//   mppi_common.hpp    Dims, GenCtx, wave reductions
//   mppi_lds.hpp       the dynamic-LDS layout of every kernel that carves one up: offsets for the kernel, the total for its launch site
//   mppi_cells.hpp     the tagged 8-byte cell: how blocks of one launch and peer devices hand values over (search, fused, exchange)
//   mppi_sample.hpp    step 1: the noise stream (gen_noise4), sample_kernel, posterior draws; opt-in: sample_colored_kernel,
//                      posterior_colored_kernel (mppi_colored.hpp: the scalar rule of the AR(1) filter)
//   mppi_rollout.hpp   steps 1b-3: rollout_cost_kernel (THE hot loop: trajectory_cost), the wavefront-per-trajectory variant
//   mppi_reduce.hpp    steps 5-6: weights_reduce_kernel
//   mppi_variance.hpp  after steps 5-6, opt-in: weighted_variance_kernel, sigma_update_kernel (mppi_covariance.hpp: the scalar rule)
//   mppi_exchange.hpp  sharded solves: peer-to-peer buffers
//   mppi_finalize.hpp  finalize_kernel (combine, normalise, SG filter, warm start, batch-1 rollout)
//   mppi_search.hpp    step 4 on the device: statistics, ESSPS / LBPS / MPO
//   mppi_fused.hpp     the whole solve as one launch (small problems)
//   mppi_topk.hpp      queries after a solve: weights, re-rolls, get_top_samples
//   mppi_env.hpp       map lookups, calc_ref_trajectory, env.step on the device
//   mppi_layout.hpp    reference layout <-> lane-major tiles
//   mppi_maps.hpp      map construction
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>  // hipExtLaunchKernel: a launch with events on its own dispatch (StageTimer)
#include <rccl/rccl.h>  // types and prototypes only: the library is dlopen()ed when a communicator is asked for

#include <cstddef>
#include <cstring>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/mppi_hip.h"
#include "host_search.hpp"
#include "mppi_fused.hpp"  // (templates only: the structs and constants of the solve's buffers)

namespace mppi {
struct TopkSel;

// ---- owners: every allocation of a handle is released by its owner's destructor

// device memory: `n` elements of T
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    // (re)allocate `count` elements; `ext_flags` != 0: hipExtMallocWithFlags (fine-grained memory)
    hipError_t alloc(size_t count, unsigned ext_flags = 0) {
        reset();
        const hipError_t e = ext_flags ? hipExtMallocWithFlags((void**)&p, sizeof(T) * count, ext_flags)
                                       : hipMalloc((void**)&p, sizeof(T) * count);
        if (e != hipSuccess) p = nullptr; else n = count;
        return e;
    }
    hipError_t alloc_set(size_t count, int byte) {  // ... and set every byte (blocking)
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : hipMemset(p, byte, sizeof(T) * count);
    }
    operator T*() const { return p; }
};

// pinned host memory, zeroed; `dev` is the device's view of it when it is mapped (looked up once, not per use)
template <class T>
struct Pinned {
    T* host = nullptr;
    T* dev = nullptr;
    Pinned() = default;
    Pinned(Pinned&& o) noexcept : host(std::exchange(o.host, nullptr)), dev(std::exchange(o.dev, nullptr)) {}
    Pinned& operator=(Pinned&& o) noexcept { std::swap(host, o.host); std::swap(dev, o.dev); return *this; }
    ~Pinned() { reset(); }
    void reset() { if (host) (void)hipHostFree(host); host = dev = nullptr; }
    hipError_t alloc(size_t count, bool mapped) {
        reset();
        hipError_t e = hipHostMalloc((void**)&host, sizeof(T) * count, mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e != hipSuccess) { host = nullptr; return e; }
        std::memset(host, 0, sizeof(T) * count);
        return mapped ? hipHostGetDevicePointer((void**)&dev, host, 0) : hipSuccess;
    }
};

// mapped flag a kernel raises when one of its polls timed out ([0]; the words after it are trace space)
struct ErrorFlag : Pinned<int> {
    int get() const { return host ? *(volatile int*)host : 0; }  // (read without synchronising)
    void clear() { if (host) *(volatile int*)host = 0; }
};

// What the statistics and search kernels write to mapped host memory (each is handed the device address of the field it fills).
struct SearchMirror {
    double single[8];          // one temperature: {min c, max c, sum e, sum e^2, sum e*c} (stats_combine_kernel)
    double grid[STATS_L * 3];  // 32 temperatures: {sum e, sum e^2, sum e*c} each (stats_multi_combine_kernel)
    double lam_next, lam_used, passes;  // a device-resident rule's temperature for the next solve, the last weights' one, its passes / probes
};
static_assert(offsetof(SearchMirror, grid) == 8 * sizeof(double), "device writes land where they did");
static_assert(offsetof(SearchMirror, lam_next) == (8 + STATS_L * 3) * sizeof(double), "device writes land where they did");

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
};
}  // namespace mppi

using namespace mppi;

struct MppiSolver {
    MppiConfig cfg{};
    Dims d{};
    int ds = 0, dc = 0;
    // generic handles whose dim_control is not 1, 2 or 4 index the per-column table core.coltab (see gen_noise4)
    bool wide = false, limits_set = true;
    int cu_count = 0;
    int lds_max = 65536;  // hipDeviceAttributeMaxSharedMemoryPerBlock
    std::string err;

    // options (mppi_set_option): what mppi_clone_state copies, as one assignment
    struct Options {
        int math_fast = 2;
        int reduce_blocks = 512;
        int reduce_chains = 0;   // "reduce_chains": 0 = by the grid size, 2 / 4 = pinned (A/B)
        int fold_mode = 0;       // "fold_path": 0 = choose by the hint; 1 = fold inside finalize when it fits; 2 = always summarize
        int fused_mode = 1;      // "fused_solve": 0 = never, 1 = small problems (default), 2 = whenever resident
        long long fused_timeout_ticks = mppi::FUSED_TIMEOUT_TICKS;  // "fused_timeout_us" (100 MHz ticks)
        int lbps_grid = 0;       // "lbps_search": 0 = Brent on the device (default), 1 = the two-grid search
        bool essps_merge0 = false;  // round 0 as one launch too (measured on par at 65 536 samples and 3.8 us SLOWER at
                                    // 262 144 — profiles/r04_experiments.md; round 1 is merged for its skip case)
        int noise_regen = 1;     // 1: Philox noise is regenerated in the kernels, never stored
        int mapping = 0;         // 0: lane per trajectory (default); 1: wavefront per trajectory (comparison)
    } opt;

    // per-solve sequence counters (the noise's solve index is core.gen.solve_idx)
    struct Seq {
        unsigned fused = 0;   // tag of the last single-launch solve's cells (fused.cells)
        unsigned brent = 0;   // probe-tag base of the next Brent search (search.brent_cells)
        unsigned round1 = 0;  // tag of the last ESSPS round-1 cells (search.round1_cells)
        unsigned p2p = 0;     // tag of the last peer-to-peer exchange (xchg.p2p_local)
    } seq;

    // The minimum cost of the last rollout as an ordered key, double-buffered: a rollout accumulates (atomicMin) into the slot
    // the rollout before it reset and resets the other one for the next -> no memset between solves.
    struct MinKey {
        DevBuf<unsigned> slots;        // two
        int idx = 0;                   // which of them the last rollout wrote
        struct Rollout { unsigned* accumulate; unsigned* reset_next; };
        const unsigned* cur() const { return slots.p + idx; }
        unsigned* cur_rw() { return slots.p + idx; }  // (refresh_min_key: the costs were replaced, not rolled out)
        Rollout begin_rollout() { idx ^= 1; return {slots.p + idx, slots.p + (idx ^ 1)}; }
        void cancel_rollout() { idx ^= 1; }  // a rollout that was begun and then not launched
    } min_key;

    // noise, costs and the state / mean the solve starts from
    struct Core {
        DevBuf<float4> noise;
        DevBuf<float> costs;
        DevBuf<float> x0;              // owned copy of the state ...
        const float* x0_cur = nullptr; // ... or a borrowed device pointer (mppi_bind_state)
        DevBuf<float> x0_used;         // the state the last rollout started from (snapshot taken by the rollout kernel)
        DevBuf<float> mean;
        DevBuf<float> mean_used;       // the mean the last rollout sampled around (snapshot taken by the rollout kernel)
        DevBuf<float> coltab;          // wide handles: per-column {sigma, lo, hi}[4R] table
        DevBuf<float> noise_std;       // [N][T][dc] copy of the noise for the wavefront-per-trajectory variant
        GenCtx gen{};                  // noise identity of the current solve ...
        bool tiles_valid = false;      // ... and whether the noise tiles hold it
        bool injected = false;         // ... because it was injected (cannot be regenerated)
    } core;

    // weights + reduction, the shard summary, finalize
    struct Reduce {
        DevBuf<float> partials;
        DevBuf<float> heads;
        DevBuf<float> summary;
        DevBuf<float> solve_stats;     // [8]: {min c, sum e, sum e^2, sum e*c, lambda used} over all shards of the last finalize
        Pinned<int> live_hint;         // mapped: partial rows the last fold saw (host-side hint)
        int last_reduce_blocks = 0;    // grid of the last weights_reduce (finalize folds its partials)
        bool summary_valid = false;    // summarize_kernel ran after the last reduce
        int GPW = 8, nchunks = 1, colsp = 128;  // float4 groups per wave, column chunks, padded row
        DevBuf<float> sg_coeffs;       // Savitzky-Golay taps (device), window sg_window (0 = filter off)
        DevBuf<float> sg_history;      // [T-1][dc] `_actions_history_for_sg` (mppi.py:160-166,441-443)
        int sg_window = 0;
    } reduce;

    // covariance adaptation (the sketch at mppi.py:400-418; capi_covariance.hip).  While `on`, the noise is drawn per COLUMN
    // from the sigma table and always materialised as tiles (the handle behaves like noise_regen = 0).
    struct Cov {
        bool on = false;
        float rate = 1.0f, floor = 1e-6f;
        DevBuf<float> sigtab;          // per-column sigma [4R], zeros past the row (wide handles: the sigma section of core.coltab)
        DevBuf<float> lim;             // {sigma_min[dc], sigma_max[dc]}
        DevBuf<float> part;            // [REDUCE_MAX_BLOCKS][colsp] partial rows of weighted_variance_kernel
        DevBuf<float> live;            // [REDUCE_MAX_BLOCKS] which of them were published
        bool ready = false;            // mppi_weights_reduce ran and mppi_finalize has not yet: the step may run
    } cov;

    // temporally correlated noise (capi_colored.hip; mppi_colored.hpp is the rule).  While `on`, the noise is drawn by
    // sample_colored_kernel and always materialised as tiles (the handle behaves like noise_regen = 0, as under cov.on).
    struct Color {
        bool on = false;
        std::vector<float> beta;       // [dc] lag-1 correlation per control dimension (empty: never set, all zero)
        DevBuf<float> tab;             // per-column {beta[4R], alpha[4R]}, zeros past the row
    } color;

    // the control-cost term (mppi.py:294-316,330-336; mppi_set_action_cost): cost_i += weight * lambda * A_i
    struct ActionCost {
        bool on = false;
        float weight = 1.0f;
        float lambda = 0.0f;           // what mppi_rollout_cost multiplies by: > 0, MPPI_LAMBDA_DEVICE, or 0 (none yet)
    } ac;

    // risk-aware solves (capi_particles.hip): while P > 0 the rollout stage evaluates every sample from every particle into
    // `costs` [P][N] and particle_fold_kernel folds the P costs of a sample into core.costs
    struct Particles {
        int P = 0;                     // start states set (0: off)
        int mode = MPPI_RISK_MEAN;     // MPPI_RISK_*
        int k = 1;                     // worst particles averaged under MPPI_RISK_CVAR (checked against P where the fold is launched)
        DevBuf<float> table;           // [MPPI_MAX_PARTICLES][ds] (native models; allocated on first use)
        DevBuf<float> costs;           // [P][N] of the last rollout (allocated on first use, grows on the set-up path)
        bool costs_valid = false;      // ... and whether a rollout / mppi_set_particle_costs has filled it for the current P
        // the map from particle to ensemble member (mppi_set_particle_members; empty: none) and its device form: the member's
        // offset into model.mlp in floats, [MPPI_MAX_PARTICLES], staged by the first rollout that uses the map
        std::vector<int> members;
        DevBuf<int32_t> member_off;
        bool member_off_valid = false;
    } part;

    // temperature: statistics passes, the device-resident ESSPS / LBPS / Brent / MPO searches
    struct Search {
        DevBuf<float> stats_part;      // [STATS_BLOCKS][max(4, STATS_L*3)]
        DevBuf<float> stats_max;       // [STATS_BLOCKS] per-block maximum cost (LBPS: the cost range)
        DevBuf<float> lams_dev;        // [3][STATS_L]: caller's grid, ESSPS round-0 grid (preset), ESSPS round-1 grid (device-written)
        Pinned<SearchMirror> mirror;   // mapped, one element
        DevBuf<float> lambda_dev;      // the temperature that search left on the device (MPPI_LAMBDA_DEVICE)
        bool lambda_dev_valid = false;
        // the rule mppi_solve applies when called with MPPI_LAMBDA_DEVICE (mppi_set_auto_lambda)
        int auto_rule = 0;
        double auto_param = 0.0, auto_lo = 0.0, auto_hi = 0.0;
        DevBuf<EsspsDev> essps_dev;    // state of the device-resident ESSPS search
        DevBuf<unsigned long long> round1_cells;  // [STATS_BLOCKS][STATS_L*3] {value, launch number}: essps_round1_kernel
        double essps_lo = 0.0, essps_hi = 0.0;    // [lam_min, lam_max] the device search's first grid was built for
        mppi::host::EsspsRange essps_range{};     // ... with its logs
        mppi::host::EsspsRoot essps_prev_host{0.0, 0.0, false};  // mppi_essps_lambda: last root (warm start of the next search) ...
        double essps_prev_lo = 0.0, essps_prev_hi = 0.0;          // ... and the range it was searched in
        DevBuf<LbpsDev> lbps_dev;      // grids of the device-resident LBPS search
        double lbps_lo = 0.0, lbps_hi = 0.0;      // [lam_min, lam_max] the preset round-0 grid was built for
        DevBuf<unsigned long long> brent_cells;   // [2][BRENT_LANES][BRENT_CELLS] tagged cells of lbps_brent_kernel
        ErrorFlag error;               // a poll of lbps_brent_kernel timed out
        int brent_drop_block = 0;      // test hook (option "search_test_drop_block"): launch one block too few
        DevBuf<mppi::host::MpoState> mpo_dev;  // MPO temperature dual + Adam moments, resident on the device (mppi_mpo_*)
        DevBuf<float> mpo_temp_dev;    // softplus(log T): the temperature of the dual's next statistics pass
    } search;

    // single-launch solve (solve_fused_kernel), allocated on first use
    struct Fused {
        DevBuf<unsigned long long> cells;  // the cells the blocks exchange through
        ErrorFlag error;
        DevBuf<double> grid0;          // [STATS_L] round-0 grid of the fused LBPS search (ESSPS: search.essps_dev->grid0)
        double grid0_lo = 0.0, grid0_hi = 0.0;
        uint64_t occ_key = 0;          // (math level, LDS bytes) the cached occupancy below belongs to
        int occ_blocks = 0;            // resident blocks of solve_fused_kernel per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor)
        int last_blocks = 0, last_spb = 0;  // grid and trajectories per block of the last mppi_solve if it was the single launch, else 0 (mppi_fused_geometry)
    } fused;

    // queries after a solve (capi_topk.hip)
    struct Topk {
        DevBuf<unsigned> hist;         // [3][TOPK_BINS] + 2 counters, kept zeroed between calls
        DevBuf<TopkSel> sel;           // [3]
        DevBuf<unsigned long long> cand;  // a power of two >= TOPK_MAX elements (the large-k sort pads to it)
    } topk;

    // lazily completed state sequence (option "lazy_state_seq"): finalize_kernel leaves {action, start state} in `b1` and
    // the batch-1 rollout of the solution rides in ONE EXTRA BLOCK of the next rollout kernel on the same stream
    // (mppi_rollout_cost) — or runs as its own one-wave kernel when somebody asks for it first (mppi_join_state_seq)
    struct Lazy {
        int on = 0;
        DevBuf<float> b1;              // [row + MPPI_MAX_DIM_STATE]
        float* pending_out = nullptr;  // where the not-yet-rolled-out state sequence of the last solve goes (or null)
        uint32_t pending_serial = 0;   // which solve that is (mppi_join_state_seq)
        hipStream_t pending_stream = nullptr;  // the stream its finalize ran on: a completion on ANOTHER stream waits for it
        Event ev;                      // (created on first use: orders such a completion behind finalize's write of b1)
        uint32_t finalize_serial = 0;
    } lazy;

    // model parameters, maps and the reference
    struct Model {
        ModelCtx ctx{};
        bool params_set = false;
        DevBuf<uint8_t> map_cells[2];
        DevBuf<uint8_t> map_pad;       // padded (and, for racing, summed) grid of the FAST lookup
        // the step table [rows][step_layout(model).stride] (mppi_models.hpp) and the rows each of its parts has been written
        // for; a part the layout does not have stays 0 and counts as complete.  publish_step_table aims ctx.ref at the table
        // once every part is there.
        DevBuf<float> ref;
        int ref_part_rows = 0;         // reference part: mppi_set_reference / mppi_ref_window
        int disc_part_rows = 0;        // disc part: mppi_set_discs
        float soft_reach = 2.0f, soft_skirt = 1.0f;  // the soft disc models' skirt as it was set (mppi_set_disc_softness)
        DevBuf<float> mlp;             // weight tables of the learned-dynamics models [mlp_members][mlp_table_floats(ds, dc)] (mppi_set_mlp:
                                       // one; mppi_set_mlp_ensemble); ctx.ref points at member mlp_nominal's
        int mlp_members = 0, mlp_nominal = 0;
        // tracking costs of the learned-dynamics models (mppi_set_mlp_reference / mppi_set_mlp_angular; mppi_models.hpp says where
        // they ride in ctx): the handle's own copy of the reference table [mlp_ref_rows][2 * ds] (0 rows: no reference), and the
        // two halves of the flags word ctx.ref_rows, which publish_mlp_flags alone composes
        DevBuf<float> mlp_ref;
        int mlp_ref_rows = 0;
        int mlp_arch = 0;              // MLP_TWO_LAYERS | MLP_TANH | MLP_RESIDUAL as mppi_set_mlp / mppi_set_mlp_ensemble gave them
        uint32_t mlp_angular = 0;      // bit m: state component m is an angle (mppi_set_mlp_angular)
        // the learned terminal value (mppi_set_mlp_value): its table [mlp_value_floats(ds)], whether one is set, its flags
        // (MLP_VALUE_*: the third part of the flags word) and its weight; publish_mlp_value aims ctx at it
        DevBuf<float> mlp_value;
        bool mlp_value_set = false;
        int mlp_value_flags = 0;
        float mlp_value_weight = 0.0f;
        // device-resident reference window (mppi_set_center_path / mppi_ref_window)
        DevBuf<float> center8;         // [n][8] centre line with sin/cos of the yaw
        DevBuf<int32_t> win_dind;      // [rows] index offsets of the window rows
        DevBuf<int32_t> path_index;    // `current_path_index`, kept on the device
        int center_n = 0, win_rows = 0;
        float win_v = 0.0f;
    } model;

    // sharded solves: peer-to-peer exchange of the shard summaries (mppi_p2p_*) or the in-library collective (mppi_comm_*)
    struct Exchange {
        DevBuf<unsigned long long> p2p_local;        // this rank's exchange buffer (fine-grained, IPC-exported)
        DevBuf<unsigned long long*> p2p_peers_dev;   // [world] every rank's buffer as mapped here
        std::vector<void*> p2p_opened;               // peer mappings, closed by the destructor
        ErrorFlag p2p_error;
        int p2p_world = 0, p2p_rank = 0, p2p_lenp = 0;
        bool p2p_connected = false, p2p_enabled = false;
        ncclComm_t comm = nullptr;     // destroyed by mppi_destroy / mppi_comm_destroy
        int comm_world = 0, comm_rank = 0;
        DevBuf<float> comm_send;       // [4 + T*dc] this shard's summary (written by summarize_kernel)
        DevBuf<float> comm_recv;       // [world][4 + T*dc]
        bool comm_enabled = false;
        Exchange() = default;
        Exchange(const Exchange&) = delete;
        ~Exchange() { for (void* pm : p2p_opened) (void)hipIpcCloseMemHandle(pm); }
    } xchg;

    // pinned staging ring for small host -> device uploads without a stream synchronisation
    struct Ring {
        static constexpr int N = 8;
        Pinned<float> slot[N];
        Event ev[N];
        size_t floats = 0;
        int next = 0;
    } ring;

    // per-stage event pairs (option "timing"; stage 4 = the deferred state sequence): start0, stop0, start1, stop1, ...
    // The rollout stage (1) is stamped by rollout_cost_kernel itself where it can be (StageTimer): `stamps` is its pool of
    // {start, end} pairs of 100 MHz wall-clock ticks, zeroed when the handle is created and again by every drain.
    struct Timers {
        static constexpr size_t STAMP_PAIRS = 8192;  // as deep as the event pool
        int mode = 0;                  // 0 off, 1 every stage, 2 the rollout stage only
        int source = 0;                // "timing_source": 0 = stamps where they apply, 1 = events everywhere
        std::vector<Event> pool[5];
        size_t used[5] = {0, 0, 0, 0, 0};
        DevBuf<unsigned long long> stamps;  // [STAMP_PAIRS][2]
        size_t stamps_used = 0;        // pairs handed to launches since the last drain
        int wall_khz = 0;              // hipDeviceAttributeWallClockRate (0: unknown, nothing is stamped)
    } timers;
};

namespace mppi {

inline int fail(mppi_handle_t h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}
#define HIP_TRY(h, expr)                                                                              \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail(h, MPPI_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

struct ModelDims { int ds, dc; };
inline bool model_dims(int model, ModelDims& md) {
    switch (model) {
    case MPPI_MODEL_PENDULUM: md = {2, 1}; return true;
    case MPPI_MODEL_CARTPOLE: md = {4, 1}; return true;
    case MPPI_MODEL_MOUNTAINCAR: md = {2, 1}; return true;
    case MPPI_MODEL_NAV2D: md = {3, 2}; return true;
    case MPPI_MODEL_RACING: md = {4, 2}; return true;
    case MPPI_MODEL_MJCARTPOLE: md = {4, 1}; return true;
    case MPPI_MODEL_GOALZONE: md = {7, 2}; return true;
    case MPPI_MODEL_MLP41: md = {4, 1}; return true;
    case MPPI_MODEL_MLP42: md = {4, 2}; return true;
    case MPPI_MODEL_NAV2D_DISCS: md = {3, 2}; return true;
    case MPPI_MODEL_RACING_DISCS: md = {4, 2}; return true;
    case MPPI_MODEL_NAV2D_DISCS_SOFT: md = {3, 2}; return true;
    case MPPI_MODEL_RACING_DISCS_SOFT: md = {4, 2}; return true;
    case MPPI_MODEL_MLP81: md = {8, 1}; return true;
    case MPPI_MODEL_MLP82: md = {8, 2}; return true;
    case MPPI_MODEL_MLP84: md = {8, 4}; return true;
    }
    return false;
}
// nav2d and its moving-disc variants: one set of dynamics, parameters, maps and host-checked preconditions
inline bool is_nav2d(int model) {
    return model == MPPI_MODEL_NAV2D || model == MPPI_MODEL_NAV2D_DISCS || model == MPPI_MODEL_NAV2D_DISCS_SOFT;
}
// parameters the dynamics of `model` read (the models without any take none)
inline int model_param_count(int model) {
    return is_racing_model(model) ? MPPI_RP_COUNT : is_nav2d(model) ? MPPI_NP_COUNT
           : model == MPPI_MODEL_GOALZONE ? MPPI_GP_COUNT : model == MPPI_MODEL_MLP41 ? MPPI_MP_COUNT41
           : model == MPPI_MODEL_MLP42 ? MPPI_MP_COUNT42 : model == MPPI_MODEL_MLP81 ? MPPI_MP8_COUNT81
           : model == MPPI_MODEL_MLP82 ? MPPI_MP8_COUNT82 : model == MPPI_MODEL_MLP84 ? MPPI_MP8_COUNT84 : 0;
}

// Times one stage with a pair of HIP events (no host synchronisation); pairs accumulate until mppi_get_timing() drains
// them.  The events ride on the stage's own dispatches (hipExtLaunchKernel): the start event on its first kernel launch,
// the stop event on its last, so a timed stage puts no marker packet on the stream and its time runs from the begin of the
// first dispatch to the end of the last.  The stage's kernels go through launch(); an untimed stage launches them exactly
// as hipLaunchKernelGGL does.  Two cases keep plain hipEventRecord markers: a stream that is being captured (both events,
// around the stage), and a stage that ends in something other than a kernel of ours (`left` = 0: the stop event, behind it).
//
// A STAMPED stage carries no events at all.  A dispatch with profiling events costs the solve about 4.5 us more than one
// without (profiles/r09_timing_markers.md), so the one launch of the rollout stage, rollout_cost_kernel, reads the 100 MHz
// wall clock itself: `stampable` stages take a pair of the handle's stamp pool (take_stamps(), handed to the kernel as an
// argument) and launch exactly as an untimed stage does.  What a stamped stage time IS: from the first instruction of block
// 0 (dispatched first) to the last instruction of the block that finishes last, (end - start) / wall-clock rate.  It lies
// INSIDE the dispatch — it leaves out what the packet processor does before the first and after the last wave — and so reads
// a little below the dispatch-bound event time and the rocprofv3 kernel time (profiles/r10_rollout_stamps.md has the
// difference).  Stamps need an uncaptured stream, a known wall-clock rate and "timing_source" = 0; a full stamp pool leaves
// the stage untimed, like a full event pool.  Every other stage and kernel keeps its events.
struct StageTimer {
    mppi_handle_t h; int stage; hipStream_t s;
    hipEvent_t start = nullptr, stop = nullptr;  // still to be placed
    bool ride = false;  // place them on the dispatches
    bool stamped = false;  // no events: the stage's kernel writes a stamp pair
    int left = 1;       // kernel launches of the stage still to come: the stop event rides on the last of them
    static hipEvent_t next(mppi_handle_t h, int stage) {
        auto& pool = h->timers.pool[stage];
        if (h->timers.used[stage] == pool.size()) {
            if (pool.size() >= 16384) return nullptr;
            Event e;
            if (hipEventCreate(&e.e) != hipSuccess) return nullptr;
            pool.push_back(std::move(e));
        }
        return pool[h->timers.used[stage]++].e;
    }
    StageTimer(mppi_handle_t h_, int stage_, hipStream_t s_, bool stampable = false) : h(h_), stage(stage_), s(s_) {
        // (stage < 0: a launch outside every stage; timing = 2: rollout_cost stage only)
        if (stage < 0 || !h->timers.mode || (h->timers.mode == 2 && stage != 1)) return;
        // (what the ext launch does with events inside a capture is left alone: a captured solve keeps its markers)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const bool eager = hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone;
        if (stampable && eager && !h->timers.source && h->timers.wall_khz > 0 && h->timers.stamps) { stamped = true; return; }
        hipEvent_t e0 = next(h, stage);
        hipEvent_t e1 = e0 ? next(h, stage) : nullptr;
        if (!e1) { if (e0) --h->timers.used[stage]; return; }  // pool full: the stage runs untimed
        ride = eager;
        stop = e1;
        if (ride) start = e0;
        else (void)hipEventRecord(e0, s);
    }
    ~StageTimer() {
        if (start) { h->timers.used[stage] -= 2; return; }  // the stage returned before its first launch: the pair goes back
        if (stop) (void)hipEventRecord(stop, s);
    }
    // The stamp pair of a stamped stage's launch, taken right before it (null: untimed, or timed with events)
    unsigned long long* take_stamps() {
        auto& t = h->timers;
        if (!stamped || t.stamps_used == MppiSolver::Timers::STAMP_PAIRS) return nullptr;
        return t.stamps.p + 2 * t.stamps_used++;
    }
    // One kernel launch of the stage: hipLaunchKernelGGL(kernel, grid, block, lds, s, a...), with the stage's events on the
    // dispatch where they are due (flags = 0).  Errors are left to the caller's hipGetLastError().
    template <class... F, class... A>
    void launch(void (*kernel)(F...), dim3 grid, dim3 block, size_t lds, const A&... a) {
        const bool last = --left == 0;
        hipEvent_t e0 = std::exchange(start, nullptr);
        hipEvent_t e1 = ride && last ? std::exchange(stop, nullptr) : nullptr;
        if (!e0 && !e1) {
            hipLaunchKernelGGL(kernel, grid, block, lds, s, a...);
            return;
        }
        std::tuple<F...> formals{a...};  // (the arguments as the kernel declares them)
        void* argv[sizeof...(F)];
        std::apply([&](auto&... f) { size_t i = 0; ((argv[i++] = (void*)&f), ...); }, formals);
        (void)hipExtLaunchKernel((const void*)kernel, grid, block, argv, lds, s, e0, e1, 0);
    }
};

// FAST kernels assume launch-uniform preconditions (see mppi_models.hpp); otherwise use FAST=false.
inline bool use_fast(mppi_handle_t h) {
    if (!h->opt.math_fast) return false;
    const int m = h->cfg.model;
    const ModelCtx& c = h->model.ctx;
    if (is_nav2d(m))
        return c.maps[0].inv_cell != 0.0f && c.pad != nullptr && c.wrap_safe != 0 && c.u_in_bounds != 0;
    if (m == MPPI_MODEL_GOALZONE) return c.wrap_safe != 0 && c.u_in_bounds != 0;
    if (is_racing_model(m))
        return c.wrap_safe != 0 && c.u_in_bounds != 0 && c.maps[0].inv_cell != 0.0f && c.pad != nullptr && c.tan_small != 0 && c.inv_L != 0.0f;
    return true;
}

// 0 = library math; 1 = polynomial fast paths; 2 = 1 + hardware sin/cos of the wrapped headings (option "math")
inline int math_level(mppi_handle_t h) { return use_fast(h) ? (h->opt.math_fast >= 2 ? 2 : 1) : 0; }

// dispatch on (model, math level); level 2 exists for the models whose trigonometric arguments are bounded by the model
// itself (wrapped headings, clamped pole angle / position): all but the pendulum, whose angle is free, and the
// MuJoCo-style cart-pole, whose open-loop instability amplifies the hardware sin/cos error 20-fold
#define MPPI_DISPATCH_HW(MODEL_, CALL)                                                                \
        case MODEL_: if (ml_ == 2) { CALL(MODEL_, 2); } else if (ml_ == 1) { CALL(MODEL_, 1); } else { CALL(MODEL_, 0); } break;
#define MPPI_DISPATCH_NOHW(MODEL_, CALL)                                                              \
        case MODEL_: if (ml_) { CALL(MODEL_, 1); } else { CALL(MODEL_, 0); } break;
#define MPPI_DISPATCH(h, CALL)                                                                        \
    do {                                                                                              \
        const int ml_ = math_level(h);                                                                \
        switch ((h)->cfg.model) {                                                                     \
        case MPPI_MODEL_GENERIC: /* only reached by mppi_finalize without a state output */          \
        MPPI_DISPATCH_NOHW(MPPI_MODEL_PENDULUM, CALL)                                                 \
        MPPI_DISPATCH_HW(MPPI_MODEL_CARTPOLE, CALL)                                                   \
        MPPI_DISPATCH_HW(MPPI_MODEL_MOUNTAINCAR, CALL)                                                \
        MPPI_DISPATCH_HW(MPPI_MODEL_NAV2D, CALL)                                                      \
        MPPI_DISPATCH_HW(MPPI_MODEL_RACING, CALL)                                                     \
        MPPI_DISPATCH_NOHW(MPPI_MODEL_MJCARTPOLE, CALL)                                               \
        MPPI_DISPATCH_HW(MPPI_MODEL_GOALZONE, CALL)                                                   \
        MPPI_DISPATCH_NOHW(MPPI_MODEL_MLP41, CALL)                                                    \
        MPPI_DISPATCH_NOHW(MPPI_MODEL_MLP42, CALL)                                                    \
        MPPI_DISPATCH_HW(MPPI_MODEL_NAV2D_DISCS, CALL)                                                \
        MPPI_DISPATCH_HW(MPPI_MODEL_RACING_DISCS, CALL)                                               \
        MPPI_DISPATCH_HW(MPPI_MODEL_NAV2D_DISCS_SOFT, CALL)                                           \
        MPPI_DISPATCH_HW(MPPI_MODEL_RACING_DISCS_SOFT, CALL)                                          \
        MPPI_DISPATCH_NOHW(MPPI_MODEL_MLP81, CALL)                                                    \
        MPPI_DISPATCH_NOHW(MPPI_MODEL_MLP82, CALL)                                                    \
        MPPI_DISPATCH_NOHW(MPPI_MODEL_MLP84, CALL)                                                    \
        }                                                                                             \
    } while (0)

// floats of one weight table of a learned-dynamics handle
inline int mlp_table_len(mppi_handle_t h) { return mlp_table_floats(h->ds, h->dc); }

inline int check_ready(mppi_handle_t h) {
    const int m = h->cfg.model;
    if (m == MPPI_MODEL_GENERIC)
        return fail(h, MPPI_E_INVALID, "generic model: dynamics/cost are host callables, this entry point is unavailable");
    if ((is_nav2d(m) || is_racing_model(m)) && !h->model.map_cells[0])
        return fail(h, MPPI_E_STATE, "obstacle map (slot 0) not uploaded");
    if (is_racing_model(m) && !h->model.map_cells[1]) return fail(h, MPPI_E_STATE, "lane map (slot 1) not uploaded");
    if (is_mlp(m) && !h->model.ctx.ref) return fail(h, MPPI_E_STATE, "no weight table: call mppi_set_mlp or mppi_set_mlp_ensemble first");
    if (is_mlp(m) && h->model.mlp_ref_rows > 0 && h->model.mlp_ref_rows < h->d.T)
        return fail(h, MPPI_E_STATE, "tracking reference has fewer rows than the horizon");
    // the step table (mppi_models.hpp): every part its layout has covers the horizon (ctx.ref is aimed at it once they do)
    const StepLayout L = step_layout(m);
    if (L.has_ref() && h->model.ref_part_rows < h->d.T)
        return fail(h, MPPI_E_STATE, "reference path not set or shorter than the horizon");
    if (L.has_discs() && h->model.disc_part_rows < 1) return fail(h, MPPI_E_STATE, "no disc table: call mppi_set_discs first");
    if (L.has_discs() && h->model.disc_part_rows < h->d.T)
        return fail(h, MPPI_E_STATE, "disc table has fewer rows than the horizon");
    // the rollout kernels keep T rows of the table in LDS (mppi_lds.hpp): refuse a horizon whose rows do not fit next to the
    // mean groups here, by name, instead of as a failed launch
    if (L.has_discs() && sizeof(float) * RolloutLds::floats(h->d.R, h->d.T, h->d.row, L.stride, true) > (size_t)h->lds_max)
        return fail(h, MPPI_E_INVALID, "horizon too long for the moving-disc model: its table rows do not fit in LDS");
    return MPPI_OK;
}

// the tag of the next use of a cell buffer (mppi_cells.hpp): 0 is skipped, it tags nothing
inline unsigned next_tag(unsigned& seq) { if (++seq == 0u) seq = 1u; return seq; }
inline P2pCtx p2p_ctx(mppi_handle_t h) {
    const auto& x = h->xchg;
    return P2pCtx{x.p2p_peers_dev, x.p2p_local, x.p2p_error.dev, x.p2p_world, x.p2p_rank, x.p2p_lenp, h->seq.p2p};
}

// RCCL through dlopen: the library stays loadable (and every unsharded path usable) on a host without RCCL.  In a
// process that already holds a librccl.so.1 (PyTorch bundles one) the loader hands back that copy.  (capi_exchange.hip)
struct RcclApi {
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    decltype(&ncclCommCount) comm_count = nullptr;        // optional (diagnostics: mppi_comm_info)
    decltype(&ncclCommUserRank) comm_user_rank = nullptr;
    bool ok = false;
};
const RcclApi& rccl();
#define RCCL_TRY(h, expr)                                                                             \
    do {                                                                                              \
        ncclResult_t _r = (expr);                                                                     \
        if (_r != ncclSuccess)                                                                        \
            return fail(h, MPPI_E_HIP, std::string(#expr) + ": " + rccl().error_string(_r));          \
    } while (0)

// capi_handle.hip: small copies through the pinned staging ring
int upload_small(mppi_handle_t h, float* dst_dev, const float* src_host, size_t floats, hipStream_t s);
int copy_small(mppi_handle_t h, void* dst, const void* src, size_t bytes, bool dst_dev, bool src_dev, hipStream_t s);
int stage_slot(mppi_handle_t h, size_t floats, float** out, hipEvent_t* ev);

// capi_model.hip
void refresh_pad(mppi_handle_t h, hipStream_t s);
int prepare_map(mppi_handle_t h, int slot, int nx, int ny, float cell, float ox, float oy);
int reserve_step_table(mppi_handle_t h, int rows);
void publish_step_table(mppi_handle_t h);
void apply_disc_softness(mppi_handle_t h, float reach, float skirt);
void publish_mlp_flags(mppi_handle_t h);      // ctx.ref_rows of a learned-dynamics handle from mlp_arch and mlp_angular
void publish_mlp_reference(mppi_handle_t h);  // aims the reference slot of ctx at mlp_ref (null while mlp_ref_rows == 0)
void publish_mlp_value(mppi_handle_t h);      // aims the value slot of ctx at mlp_value with its weight (null while none is set)

// the per-column sigma table the sampler reads (see MppiSolver::Cov)
inline float* sigma_table(mppi_handle_t h) { return h->wide ? h->core.coltab.p : h->cov.sigtab.p; }
// the noise of this handle exists as materialised tiles only, whatever option "noise_regen" says: sigma comes per step from
// the adapted table, or the draw carries a filter along the horizon (the regenerating consumers know neither)
inline bool tiles_only(mppi_handle_t h) { return h->cov.on || h->color.on; }
// regenerate the noise in registers?  Not when it was injected, nor when sigma comes per column from a table
inline bool regen_noise(mppi_handle_t h) { return h->opt.noise_regen && !h->core.injected && !h->wide && !tiles_only(h); }

// capi_covariance.hip
int cov_alloc(mppi_handle_t h);
int fill_sigma_table(mppi_handle_t h, const float* sigmas, int n);

// capi_colored.hip: the correlated forms of the tile draw (one launch of the stage `tm`) and of the posterior draw
int sample_colored(mppi_handle_t h, StageTimer& tm);
int posterior_colored(mppi_handle_t h, const GenCtx& g, const float* loc_dev, int k, float* samples_out_dev, hipStream_t s);

// capi_solve.hip
int resolve_lambda(mppi_handle_t h, float lambda, const float** lam_dev);
int need_tiles(mppi_handle_t h, hipStream_t s);
int flush_state_seq(mppi_handle_t h, hipStream_t s);
// Before anything that changes which kernel variant MPPI_DISPATCH picks or what the model context holds (math level,
// mapping, maps, model parameters): complete a pending state sequence with the settings of the solve it belongs to, on the
// stream that solve ran on.
inline int settle_state_seq(mppi_handle_t h) { return h->lazy.pending_out ? flush_state_seq(h, h->lazy.pending_stream) : MPPI_OK; }

// capi_particles.hip: the rollout stage while particles are set (rollout from every particle, then the fold)
int rollout_particles(mppi_handle_t h, hipStream_t s);
int clone_particles(mppi_handle_t dst, mppi_handle_t src);

// capi_search.hip
int essps_prepare(mppi_handle_t h, double lam_min, double lam_max);
int mpo_upload(mppi_handle_t h, double lambda0, double epsilon, double lr, bool lambda_too);

// capi_topk.hip
int topk_alloc(mppi_handle_t h);

}  // namespace mppi
