// capi_handle.hip — C ABI (include/mppi_hip.h): the handle's life cycle, options, timing, the mean and the state.
// Host-side only; the handle and the helpers the units share are in mppi_handle.hpp.  No torch, no exceptions across the
// boundary.
#include <new>

#include "mppi_handle.hpp"

namespace mppi {

// Pinned staging slot of at least `floats` floats; waits (rarely) for the slot's previous upload.
int stage_slot(mppi_handle_t h, size_t floats, float** out, hipEvent_t* ev) {
    auto& r = h->ring;
    if (floats > r.floats) {
        for (int i = 0; i < r.N; ++i) {
            if (r.ev[i].e) HIP_TRY(h, hipEventSynchronize(r.ev[i].e));
            HIP_TRY(h, r.slot[i].alloc(floats, false));
            if (!r.ev[i].e) HIP_TRY(h, hipEventCreateWithFlags(&r.ev[i].e, hipEventDisableTiming));
        }
        r.floats = floats;
    }
    const int i = r.next;
    r.next = (i + 1) % r.N;
    HIP_TRY(h, hipEventSynchronize(r.ev[i].e));  // no-op unless 8 uploads are still in flight
    *out = r.slot[i].host;
    *ev = r.ev[i].e;
    return MPPI_OK;
}

// host -> device upload of a few floats through the pinned ring: asynchronous, no host wait
int upload_small(mppi_handle_t h, float* dst_dev, const float* src_host, size_t floats, hipStream_t s) {
    float* st = nullptr; hipEvent_t ev = nullptr;
    if (int rc = stage_slot(h, std::max<size_t>(floats, 64), &st, &ev)) return rc;
    std::memcpy(st, src_host, sizeof(float) * floats);
    HIP_TRY(h, hipMemcpyAsync(dst_dev, st, sizeof(float) * floats, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(ev, s));
    return MPPI_OK;
}

// device <-> device / device -> host copies of small vectors
int copy_small(mppi_handle_t h, void* dst, const void* src, size_t bytes, bool dst_dev, bool src_dev, hipStream_t s) {
    if (dst_dev && !src_dev) return upload_small(h, (float*)dst, (const float*)src, bytes / sizeof(float), s);
    const hipMemcpyKind kind = dst_dev ? hipMemcpyDeviceToDevice : (src_dev ? hipMemcpyDeviceToHost : hipMemcpyHostToHost);
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, kind, s));
    if (!dst_dev) HIP_TRY(h, hipStreamSynchronize(s));
    return MPPI_OK;
}

}  // namespace mppi

namespace {

// `count` elements of src -> dst (device to device, blocking); a buffer missing on either side copies nothing
template <class T>
int clone_buf(mppi_handle_t h, T* dst, const T* src, size_t count) {
    if (!count || !src || !dst) return MPPI_OK;
    HIP_TRY(h, hipMemcpy(dst, src, sizeof(T) * count, hipMemcpyDeviceToDevice));
    return MPPI_OK;
}

// mean device time [ms] and count of the event pairs of `stage` since the last drain: {-1, 0} without any
int drain_timing(mppi_handle_t h, int stage, float* mean_ms, float* count) {
    *mean_ms = -1.0f;
    *count = 0.0f;
    const auto& pool = h->timers.pool[stage];
    const size_t pairs = h->timers.used[stage] / 2;
    double sum = 0.0;
    for (size_t p = 0; p < pairs; ++p) {
        float ms = 0.0f;
        HIP_TRY(h, hipEventSynchronize(pool[2 * p + 1].e));
        HIP_TRY(h, hipEventElapsedTime(&ms, pool[2 * p].e, pool[2 * p + 1].e));
        sum += ms;
    }
    h->timers.used[stage] = 0;
    // the rollout stage's stamp pairs (StageTimer): ticks of the wall clock, written by the kernels themselves.  They join
    // the event pairs in the one mean; the used pairs are zeroed again (the end stamp is an atomicMax).
    auto& t = h->timers;
    size_t stamped = 0;
    if (stage == 1 && t.stamps_used) {
        std::vector<unsigned long long> st(2 * t.stamps_used);
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, hipMemcpy(st.data(), t.stamps, sizeof(unsigned long long) * st.size(), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemset(t.stamps, 0, sizeof(unsigned long long) * st.size()));
        t.stamps_used = 0;
        for (size_t p = 0; p < st.size(); p += 2) {
            if (!st[p] || st[p + 1] < st[p]) continue;  // (a launch that never ran)
            sum += (double)(st[p + 1] - st[p]) / (double)t.wall_khz;
            ++stamped;
        }
    }
    const size_t n = pairs + stamped;
    if (n) { *mean_ms = (float)(sum / (double)n); *count = (float)n; }
    return MPPI_OK;
}

}  // namespace

extern "C" {

const char* mppi_version(void) { return "mppi_hip 0.3.0 (gfx950, wave64, lane-per-trajectory)"; }
int mppi_abi_version(void) { return MPPI_ABI_VERSION; }

int mppi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* mppi_last_error(mppi_handle_t h) { return h ? h->err.c_str() : "null handle"; }

int mppi_create(const MppiConfig* cfg, mppi_handle_t* out) {
    if (!cfg || !out) return MPPI_E_INVALID;
    *out = nullptr;
    ModelDims md{};
    if (cfg->model == MPPI_MODEL_GENERIC) {
        // any control dimension: 1, 2 and 4 index the launch constants, every other value the per-column table
        if (cfg->dim_state < 1 || cfg->dim_control < 1 || cfg->dim_control > MPPI_MAX_DIM_CONTROL_GENERIC)
            return MPPI_E_INVALID;
        md = {cfg->dim_state, cfg->dim_control};
    } else {
        if (!model_dims(cfg->model, md)) return MPPI_E_INVALID;
        if (cfg->dim_state != md.ds || cfg->dim_control != md.dc) return MPPI_E_INVALID;
    }
    if (cfg->horizon < 1 || cfg->num_samples < 1) return MPPI_E_INVALID;
    if (mppi_device_count() <= 0) return MPPI_E_NODEVICE;
    MppiSolver* h = new (std::nothrow) MppiSolver();
    if (!h) return MPPI_E_INVALID;
    h->cfg = *cfg;
    h->ds = md.ds; h->dc = md.dc;
    Dims& d = h->d;
    d.N = cfg->num_samples;
    d.tiles = (d.N + 63) / 64;
    d.sample_offset = cfg->sample_offset;
    d.inherit_count = cfg->inherit_count;
    d.T = cfg->horizon;
    d.row = d.T * md.dc;
    d.R = (d.row + 3) / 4;
    for (int k = 0; k < MPPI_MAX_DIM_CONTROL; ++k) {
        d.u_min[k] = cfg->u_min[k]; d.u_max[k] = cfg->u_max[k]; d.sigma[k] = cfg->sigmas[k];
    }
    h->wide = cfg->model == MPPI_MODEL_GENERIC && md.dc != 1 && md.dc != 2 && md.dc != 4;
    // Every wave owns 8 float4 groups of a 32-group column chunk; longer rows (T*dim_control > 128) take more chunks
    // (grid.y), each regenerating / reading only its own groups.  (Rounds 1-3 gave such rows 32 groups per wave: 128
    // accumulators per lane, 163-231 VGPRs and 15-66 SGPR spills; the chunked form computes the same sums — a column is
    // owned by one wave either way and accumulates its tiles in the same order — without that kernel.)
    auto& red = h->reduce;
    red.GPW = 8;
    const int chg = red.GPW * (BLOCK / WAVE);  // float4 groups per column chunk
    red.nchunks = (d.R + chg - 1) / chg;
    red.colsp = red.nchunks * chg * 4;
    *out = h;  // so that the caller can read the error and destroy on failure
    HIP_TRY(h, hipSetDevice(cfg->device));
    auto& c = h->core;
    HIP_TRY(h, c.noise.alloc_set((size_t)d.tiles * d.R * 64, 0));
    HIP_TRY(h, c.costs.alloc((size_t)d.N));
    HIP_TRY(h, h->min_key.slots.alloc_set(2, 0xFF));
    const size_t x0_floats = (size_t)std::max(md.ds, MPPI_MAX_DIM_STATE);
    HIP_TRY(h, c.x0.alloc_set(x0_floats, 0));
    c.x0_cur = c.x0;
    HIP_TRY(h, c.x0_used.alloc_set(x0_floats, 0));
    c.gen = GenCtx{(uint32_t)cfg->seed, (uint32_t)(cfg->seed >> 32), 0u};
    d.dc = md.dc;
    HIP_TRY(h, c.mean.alloc_set((size_t)d.row, 0));  // mppi.py:157
    HIP_TRY(h, c.mean_used.alloc_set((size_t)d.row, 0));
    HIP_TRY(h, red.solve_stats.alloc_set(8, 0));
    if (int rc = topk_alloc(h)) return rc;
    const int max_blocks = 2048;
    HIP_TRY(h, red.partials.alloc((size_t)max_blocks * red.colsp));
    HIP_TRY(h, red.heads.alloc((size_t)max_blocks * 4));
    HIP_TRY(h, red.summary.alloc((size_t)(MPPI_SUMMARY_HEAD + d.row)));
    auto& se = h->search;
    HIP_TRY(h, se.stats_part.alloc((size_t)STATS_L * 3 * STATS_BLOCKS));
    HIP_TRY(h, se.round1_cells.alloc_set((size_t)STATS_L * 3 * STATS_BLOCKS, 0));
    HIP_TRY(h, se.mirror.alloc(1, true));
    HIP_TRY(h, se.mpo_dev.alloc(1));
    HIP_TRY(h, se.mpo_temp_dev.alloc(1));
    HIP_TRY(h, se.lbps_dev.alloc(1));
    HIP_TRY(h, se.stats_max.alloc(STATS_BLOCKS));
    HIP_TRY(h, se.brent_cells.alloc_set((size_t)2 * BRENT_LANES * BRENT_CELLS, 0));
    HIP_TRY(h, se.error.alloc(16, true));
    HIP_TRY(h, hipDeviceGetAttribute(&h->lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device));
    HIP_TRY(h, se.lams_dev.alloc((size_t)3 * STATS_L));
    HIP_TRY(h, se.essps_dev.alloc(1));
    HIP_TRY(h, se.lambda_dev.alloc(1));
    HIP_TRY(h, red.live_hint.alloc(1, true));
    std::memset(&h->model.ctx, 0, sizeof(h->model.ctx));
    if (is_soft_discs(cfg->model)) apply_disc_softness(h, 2.0f, 1.0f);
    if (h->wide) {
        HIP_TRY(h, c.coltab.alloc(12 * (size_t)d.R));
        h->limits_set = false;
        if (md.dc <= MPPI_MAX_DIM_CONTROL)  // the config arrays hold all of it (dim_control = 3)
            if (int rc = mppi_set_control_limits(h, cfg->u_min, cfg->u_max, cfg->sigmas, md.dc)) return rc;
    } else {  // the per-step sigma table of the covariance adaptation (wide handles: the sigma section of coltab)
        HIP_TRY(h, h->cov.sigtab.alloc(4 * (size_t)d.R));
        if (int rc = fill_sigma_table(h, cfg->sigmas, md.dc)) return rc;
    }
    if (int rc = mpo_upload(h, 1.0, 0.1, 0.2, false)) return rc;  // mppi.py:191-200
    HIP_TRY(h, hipDeviceGetAttribute(&h->cu_count, hipDeviceAttributeMultiprocessorCount, cfg->device));
    // the rollout stage's stamp pool (StageTimer); without a wall-clock rate the stage keeps its events
    if (hipDeviceGetAttribute(&h->timers.wall_khz, hipDeviceAttributeWallClockRate, cfg->device) != hipSuccess) h->timers.wall_khz = 0;
    if (h->timers.wall_khz > 0) HIP_TRY(h, h->timers.stamps.alloc_set(2 * MppiSolver::Timers::STAMP_PAIRS, 0));
    HIP_TRY(h, hipDeviceSynchronize());
    return MPPI_OK;
}

// u_min / u_max / sigmas of all dim_control controls (host arrays).  Required once for generic handles with more
// than MPPI_MAX_DIM_CONTROL controls (the config arrays hold four); replaces the bounds of any handle.  Synchronises.
int mppi_set_control_limits(mppi_handle_t h, const float* u_min, const float* u_max, const float* sigmas, int n) {
    if (!h || !u_min || !u_max || !sigmas || n != h->dc) return fail(h, MPPI_E_INVALID, "control limits: need dim_control values each");
    for (int k = 0; k < n; ++k)
        if (!(u_min[k] <= u_max[k]) || !(sigmas[k] >= 0.0f)) return fail(h, MPPI_E_INVALID, "control limits: need u_min <= u_max, sigma >= 0");
    if (h->cfg.model != MPPI_MODEL_GENERIC && h->model.params_set)  // the fast-path preconditions were derived from the old bounds
        return fail(h, MPPI_E_STATE, "control limits of a native model must be set before its parameters");
    Dims& d = h->d;
    for (int k = 0; k < std::min(n, (int)MPPI_MAX_DIM_CONTROL); ++k) {
        d.u_min[k] = h->cfg.u_min[k] = u_min[k];
        d.u_max[k] = h->cfg.u_max[k] = u_max[k];
        d.sigma[k] = h->cfg.sigmas[k] = sigmas[k];
    }
    if (h->wide) {
        const size_t C = 4 * (size_t)d.R;
        std::vector<float> tab(3 * C, 0.0f);
        for (int f = 0; f < d.row; ++f) {
            tab[f] = sigmas[f % n]; tab[C + f] = u_min[f % n]; tab[2 * C + f] = u_max[f % n];
        }
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, hipMemcpy(h->core.coltab, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
        h->limits_set = true;
        h->core.tiles_valid = h->core.tiles_valid && h->core.injected;
    } else {  // (the per-step sigma table starts over from the new `sigmas`: an adapted table is reset, tiles drawn from it are stale)
        if (int rc = fill_sigma_table(h, sigmas, n)) return rc;
        h->core.tiles_valid = h->core.tiles_valid && h->core.injected;
    }
    return MPPI_OK;
}

// Every buffer, pinned page, event and peer mapping belongs to an owner in the handle; the communicator is RCCL's.
int mppi_destroy(mppi_handle_t h) {
    if (!h) return MPPI_E_INVALID;
    if (h->xchg.comm) (void)rccl().comm_destroy(h->xchg.comm);
    delete h;
    return MPPI_OK;
}

// copy.deepcopy(solver) (the reference is a plain nn.Module, mppi.py:16: every tensor it holds is copied with it): make `dst`
// — a handle created from the same MppiConfig — continue exactly like `src` from here: warm start, noise identity, costs and
// minimum of the last solve (queries), Savitzky-Golay history, the temperature and every device-resident search / dual
// state, model parameters, maps, reference window and path index, the weight table of a learned model, options.  Not copied: the single-launch solve's, the Brent
// search's, the ESSPS round-1 and the exchange's tags and buffers, the timers.  Set-up path: synchronises the device.
int mppi_clone_state(mppi_handle_t dst, mppi_handle_t src) {
    if (!dst || !src || dst == src) return fail(dst, MPPI_E_INVALID, "clone_state: two distinct handles");
    const MppiConfig &a = dst->cfg, &b = src->cfg;
    if (a.model != b.model || a.horizon != b.horizon || a.dim_state != b.dim_state || a.dim_control != b.dim_control ||
        a.num_samples != b.num_samples || a.sample_offset != b.sample_offset || a.inherit_count != b.inherit_count ||
        a.device != b.device)
        return fail(dst, MPPI_E_INVALID, "clone_state: the handles were created from different configurations");
    if (int rc = settle_state_seq(src)) return rc;
    if (int rc = settle_state_seq(dst)) return rc;
    HIP_TRY(dst, hipDeviceSynchronize());
    const Dims& d = src->d;
    dst->cfg = src->cfg; dst->d = src->d; dst->wide = src->wide; dst->limits_set = src->limits_set;
#define CLONE(field) do { if (int rc = clone_buf(dst, dst->field.p, src->field.p, src->field.n)) return rc; } while (0)
    auto &dc = dst->core, &sc = src->core;
    if (sc.tiles_valid) CLONE(core.noise);
    CLONE(core.costs);
    CLONE(min_key.slots);
    if (int rc = clone_buf(dst, dc.x0.p, sc.x0_cur, (size_t)src->ds)) return rc;  // (a borrowed state becomes an owned copy)
    dc.x0_cur = dc.x0;
    CLONE(core.x0_used);
    CLONE(core.coltab);
    CLONE(cov.sigtab);
    if (src->cov.on) {  // covariance adaptation: the settings (the table itself is one of the two buffers above)
        if (int rc = cov_alloc(dst)) return rc;
        CLONE(cov.lim);
    }
    dst->cov.on = src->cov.on; dst->cov.rate = src->cov.rate; dst->cov.floor = src->cov.floor; dst->cov.ready = false;
    // the noise correlation: the setting (its table is rebuilt from it; dst's tile bookkeeping follows below)
    if (src->color.on || dst->color.on)
        if (int rc = mppi_set_noise_correlation(dst, src->color.on ? src->color.beta.data() : nullptr)) return rc;
    dst->ac = src->ac;  // the control-cost term: switch, weight and the temperature of the next stand-alone rollout
    if (int rc = clone_particles(dst, src)) return rc;  // risk-aware solves: table, count, risk measure, the last matrix
    CLONE(core.mean);
    CLONE(core.mean_used);
    CLONE(reduce.solve_stats);
    CLONE(reduce.summary);
    CLONE(search.mpo_dev);
    CLONE(search.mpo_temp_dev);
    CLONE(search.lbps_dev);
    CLONE(search.lams_dev);
    CLONE(search.essps_dev);
    CLONE(search.lambda_dev);
    if (src->fused.grid0 && !dst->fused.grid0) HIP_TRY(dst, dst->fused.grid0.alloc(STATS_L));
    CLONE(fused.grid0);
    dst->min_key.idx = src->min_key.idx; dc.gen = sc.gen; dc.tiles_valid = sc.tiles_valid; dc.injected = sc.injected;
    dst->opt = src->opt;
    auto &ds = dst->search, &ss = src->search;
    ds.auto_rule = ss.auto_rule; ds.auto_param = ss.auto_param; ds.auto_lo = ss.auto_lo; ds.auto_hi = ss.auto_hi;
    ds.lbps_lo = ss.lbps_lo; ds.lbps_hi = ss.lbps_hi; dst->fused.grid0_lo = src->fused.grid0_lo; dst->fused.grid0_hi = src->fused.grid0_hi;
    ds.essps_lo = ss.essps_lo; ds.essps_hi = ss.essps_hi; ds.essps_range = ss.essps_range;
    ds.essps_prev_host = ss.essps_prev_host; ds.essps_prev_lo = ss.essps_prev_lo; ds.essps_prev_hi = ss.essps_prev_hi;
    ds.lambda_dev_valid = ss.lambda_dev_valid;
    ds.mirror.host->lam_next = ss.mirror.host->lam_next; ds.mirror.host->lam_used = ss.mirror.host->lam_used;
    ds.mirror.host->passes = ss.mirror.host->passes;
    auto &dr = dst->reduce, &sr = src->reduce;
    dr.last_reduce_blocks = 0;            // the partial rows of src's last reduction are not copied ...
    dr.summary_valid = sr.summary_valid || sr.last_reduce_blocks > 0;
    if (!sr.summary_valid && sr.last_reduce_blocks > 0) {  // ... so a finalize on dst alone would find nothing: copy them after all
        CLONE(reduce.partials);
        CLONE(reduce.heads);
        dr.last_reduce_blocks = sr.last_reduce_blocks; dr.summary_valid = false;
    }
    // Savitzky-Golay filter
    dr.sg_window = 0;
    if (sr.sg_coeffs && sr.sg_history) {
        if (!dr.sg_coeffs) HIP_TRY(dst, dr.sg_coeffs.alloc(sr.sg_coeffs.n));
        if (!dr.sg_history) HIP_TRY(dst, dr.sg_history.alloc(sr.sg_history.n));
        CLONE(reduce.sg_coeffs);
        CLONE(reduce.sg_history);
        dr.sg_window = sr.sg_window;
    }
    // lazily completed state sequences: the option, not a pending rollout (both were settled above)
    if (src->lazy.on && !dst->lazy.b1) HIP_TRY(dst, dst->lazy.b1.alloc((size_t)d.row + MPPI_MAX_DIM_STATE));
    dst->lazy.on = src->lazy.on;
    // model context: parameters and flags by value, every pointer re-aimed at dst's own copy
    auto &dm = dst->model, &sm = src->model;
    const ModelCtx old = dm.ctx;
    dm.ctx = sm.ctx;
    dm.params_set = sm.params_set;
    for (int slot = 0; slot < 2; ++slot) {
        dm.ctx.maps[slot].cells = old.maps[slot].cells;
        if (!sm.map_cells[slot]) { dm.ctx.maps[slot] = old.maps[slot]; continue; }
        const MapView& m = sm.ctx.maps[slot];
        if (int rc = prepare_map(dst, slot, m.nx, m.ny, m.cell, m.ox, m.oy)) return rc;
        if (int rc = clone_buf(dst, dm.map_cells[slot].p, sm.map_cells[slot].p, (size_t)m.nx * m.ny)) return rc;
    }
    dm.ctx.ref = nullptr; dm.ctx.ref_rows = 0;
    dm.ref_part_rows = dm.disc_part_rows = 0;
    if (sm.ref) {  // the step table with the rows of each part (the disc count was copied with ctx)
        if (int rc = reserve_step_table(dst, (int)(sm.ref.n / (size_t)step_layout(src->cfg.model).stride))) return rc;
        if (int rc = clone_buf(dst, dm.ref.p, sm.ref.p, sm.ref.n)) return rc;
        dm.ref_part_rows = sm.ref_part_rows; dm.disc_part_rows = sm.disc_part_rows;
        publish_step_table(dst);
    }
    dm.soft_reach = sm.soft_reach; dm.soft_skirt = sm.soft_skirt;  // (the coefficients they stand for were copied with ctx)
    if (sm.mlp && sm.ctx.ref) {  // learned dynamics: every member's weight table, the nominal index, the flags that ride in ref_rows
        if (dm.mlp.n != sm.mlp.n) HIP_TRY(dst, dm.mlp.alloc(sm.mlp.n));
        CLONE(model.mlp);
        dm.mlp_members = sm.mlp_members; dm.mlp_nominal = sm.mlp_nominal;
        dm.ctx.ref = dm.mlp.p + (sm.ctx.ref - sm.mlp.p);
    }
    if (is_mlp(src->cfg.model)) {  // the tracking reference and the two halves of the flags word (set before or after the weights)
        dm.mlp_arch = sm.mlp_arch; dm.mlp_angular = sm.mlp_angular;
        publish_mlp_flags(dst);
        dm.mlp_ref_rows = 0;
        if (sm.mlp_ref_rows > 0) {
            const size_t floats = (size_t)sm.mlp_ref_rows * 2 * (size_t)src->ds;
            if (dm.mlp_ref.n < floats) HIP_TRY(dst, dm.mlp_ref.alloc(floats));
            if (int rc = clone_buf(dst, dm.mlp_ref.p, sm.mlp_ref.p, floats)) return rc;
            dm.mlp_ref_rows = sm.mlp_ref_rows;
        }
        publish_mlp_reference(dst);
        // the learned terminal value: table, flags and weight
        dm.mlp_value_set = false;
        if (sm.mlp_value_set) {
            if (dm.mlp_value.n < sm.mlp_value.n) HIP_TRY(dst, dm.mlp_value.alloc(sm.mlp_value.n));
            if (int rc = clone_buf(dst, dm.mlp_value.p, sm.mlp_value.p, sm.mlp_value.n)) return rc;
            dm.mlp_value_set = true;
        }
        dm.mlp_value_flags = sm.mlp_value_flags; dm.mlp_value_weight = sm.mlp_value_weight;
        publish_mlp_value(dst);
    }
    if (sm.center_n) {
        HIP_TRY(dst, dm.center8.alloc(sm.center8.n));
        HIP_TRY(dst, dm.win_dind.alloc(sm.win_dind.n));
        if (!dm.path_index) HIP_TRY(dst, dm.path_index.alloc(1));
        CLONE(model.center8);
        CLONE(model.win_dind);
        CLONE(model.path_index);
        dm.center_n = sm.center_n; dm.win_rows = sm.win_rows; dm.win_v = sm.win_v;
    }
#undef CLONE
    refresh_pad(dst, nullptr);  // the padded grid of the fast lookups, rebuilt from dst's own maps
    HIP_TRY(dst, hipDeviceSynchronize());
    return MPPI_OK;
}

int mppi_set_mean(mppi_handle_t h, const float* mean, int on_device, void* stream) {
    if (!h || !mean) return fail(h, MPPI_E_INVALID, "null");
    return copy_small(h, h->core.mean, mean, sizeof(float) * (size_t)h->d.row, true, on_device != 0, (hipStream_t)stream);
}
int mppi_get_mean(mppi_handle_t h, float* out, int on_device, void* stream) {
    if (!h || !out) return fail(h, MPPI_E_INVALID, "null");
    return copy_small(h, out, h->core.mean, sizeof(float) * (size_t)h->d.row, on_device != 0, true, (hipStream_t)stream);
}
int mppi_set_state(mppi_handle_t h, const float* x0, int on_device, void* stream) {
    if (!h || !x0) return fail(h, MPPI_E_INVALID, "null");
    h->core.x0_cur = h->core.x0;
    return copy_small(h, h->core.x0, x0, sizeof(float) * (size_t)h->ds, true, on_device != 0, (hipStream_t)stream);
}
int mppi_bind_state(mppi_handle_t h, const float* x0_dev) {
    if (!h || !x0_dev) return fail(h, MPPI_E_INVALID, "null");
    h->core.x0_cur = x0_dev;
    return MPPI_OK;
}

int mppi_set_option(mppi_handle_t h, const char* key, int64_t value) {
    if (!h || !key) return MPPI_E_INVALID;
    const std::string k(key);
    auto& o = h->opt;
    if (k == "math" || k == "mapping") { if (int rc = settle_state_seq(h)) return rc; }  // (a pending state sequence keeps ITS solve's variant)
    if (k == "math") { o.math_fast = value < 0 ? 0 : value > 2 ? 2 : (int)value; return MPPI_OK; }
    if (k == "reduce_blocks") { o.reduce_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(value, 2048)); return MPPI_OK; }
    if (k == "timing") { h->timers.mode = (int)value; return MPPI_OK; }
    if (k == "timing_source") { h->timers.source = value ? 1 : 0; return MPPI_OK; }  // 1: events for every stage (A/B of the stamps)
    if (k == "mapping" && value && h->ac.on) return fail(h, MPPI_E_INVALID, "the control-cost term is not available with mapping = 1");
    if (k == "mapping" && value && h->part.P > 0) return fail(h, MPPI_E_INVALID, "particles are not available with mapping = 1");
    if (k == "mapping") { o.mapping = value ? 1 : 0; return MPPI_OK; }
    if (k == "essps_cold") {  // the next ESSPS search (device chain and host loop) starts from the geometric grid
        h->search.essps_lo = h->search.essps_hi = 0.0;
        h->search.essps_prev_host.warm = false;
        return MPPI_OK;
    }
    if (k == "reduce_chains") { o.reduce_chains = value == 2 ? 2 : value == 4 ? 4 : 0; return MPPI_OK; }
    if (k == "fused_solve") { o.fused_mode = value < 0 ? 0 : value > 2 ? 2 : (int)value; return MPPI_OK; }
    if (k == "fused_timeout_us") {  // poll budget of the single-launch solve (default 20 000 us; 100 MHz ticks inside)
        if (value < 100 || value > 60000000) return fail(h, MPPI_E_INVALID, "fused_timeout_us: 100 us .. 60 s");
        o.fused_timeout_ticks = (long long)value * 100;
        return MPPI_OK;
    }
    if (k == "fused_rearm") { h->fused.error.clear(); return MPPI_OK; }  // after a timed-out poll demoted the handle: allow the single launch again
    if (k == "lazy_state_seq") {  // see mppi_join_state_seq
        if (value && !h->lazy.b1) HIP_TRY(h, h->lazy.b1.alloc((size_t)h->d.row + MPPI_MAX_DIM_STATE));
        h->lazy.on = value ? 1 : 0;
        return MPPI_OK;
    }
    if (k == "lbps_search") { o.lbps_grid = value ? 1 : 0; return MPPI_OK; }  // what mppi_solve's LBPS rule runs: 0 Brent (default), 1 grids
    if (k == "search_test_drop_block") { h->search.brent_drop_block = value ? 1 : 0; return MPPI_OK; }
    if (k == "search_rearm") { h->search.error.clear(); return MPPI_OK; }
    if (k == "essps_merge0") { o.essps_merge0 = value != 0; return MPPI_OK; }  // A/B: round 0 of the ESSPS chain as one launch
    if (k == "fold_path") { o.fold_mode = (value >= 0 && value <= 2) ? (int)value : 0; return MPPI_OK; }
    if ((k == "exchange_p2p" || k == "exchange_comm") && value && h->cov.on)
        return fail(h, MPPI_E_INVALID, "covariance adaptation is not available for sharded solves (the variance would need a second exchange)");
    if (k == "exchange_p2p") {  // sharded solves: summaries travel through the peer-to-peer buffer, no collective
        if (value && !h->xchg.p2p_connected) return fail(h, MPPI_E_STATE, "exchange_p2p: call mppi_p2p_alloc / mppi_p2p_connect first");
        h->xchg.p2p_enabled = value != 0;
        return MPPI_OK;
    }
    if (k == "exchange_comm") {  // sharded solves: mppi_weights_reduce all_gathers the summaries itself (RCCL, same stream)
        if (value && !h->xchg.comm) return fail(h, MPPI_E_STATE, "exchange_comm: call mppi_comm_init first");
        h->xchg.comm_enabled = value != 0;
        return MPPI_OK;
    }
    if (k == "noise_regen") {  // (under covariance adaptation or a noise correlation the tiles are the noise whatever this says: they stay)
        o.noise_regen = value ? 1 : 0;
        h->core.tiles_valid = h->core.tiles_valid && (h->core.injected || tiles_only(h));
        return MPPI_OK;
    }
    return fail(h, MPPI_E_INVALID, "unknown option " + k);
}

int mppi_get_math_level(mppi_handle_t h, int* level_out) {
    if (!h || !level_out) return fail(h, MPPI_E_INVALID, "null");
    *level_out = math_level(h);
    return MPPI_OK;
}

// mean device time [ms] and launch count of the stand-alone state-sequence kernel (mppi_join_state_seq; the rollouts that
// rode in a rollout launch are not separate kernels) since the last call (option "timing" = 1)
int mppi_get_state_seq_timing(mppi_handle_t h, float* out2) {
    if (!h || !out2) return MPPI_E_INVALID;
    return drain_timing(h, 4, &out2[0], &out2[1]);
}

int mppi_get_timing(mppi_handle_t h, float* out) {
    if (!h || !out) return MPPI_E_INVALID;
    for (int i = 0; i < 4; ++i)
        if (int rc = drain_timing(h, i, &out[i], &out[4 + i])) return rc;
    return MPPI_OK;
}

}  // extern "C"
