// capi_particles.hip — C ABI (include/mppi_hip.h): risk-aware solves.  The table of start states ("particles"), the risk
// measure, the rollout stage while particles are set (rollout_particles_kernel from every particle, then particle_fold_kernel)
// and the [P][N] cost matrix's get / set, and the map from particle to ensemble member of the learned-dynamics models
// (mppi_set_particle_members).  The kernels are in mppi_particles.hpp; this unit is the only one that launches them.
#include <algorithm>
#include <cmath>

#include "mppi_handle.hpp"
#include "mppi_particles.hpp"

namespace mppi {

// the [P][N] matrix for `P` particles: allocated on first use, grows (blocking: earlier launches may still read it) only
static int reserve_particle_costs(mppi_handle_t h, int P) {
    const size_t need = (size_t)P * (size_t)h->d.N;
    if (h->part.costs.n >= need) return MPPI_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, h->part.costs.alloc(need));
    h->part.costs_valid = false;
    return MPPI_OK;
}

// particle_fold_kernel over the matrix as it stands: costs[N] and the minimum key (one launch of the stage `tm`)
static int fold_particles(mppi_handle_t h, StageTimer& tm) {
    const auto& p = h->part;
    if (p.mode == MPPI_RISK_CVAR && (p.k < 1 || p.k > p.P))
        return fail(h, MPPI_E_INVALID, "risk measure: CVAR needs 1 <= k <= P (mppi_set_risk / mppi_set_particles)");
    const auto mk = h->min_key.begin_rollout();
    const unsigned grid = (unsigned)std::min<int64_t>((h->d.N + BLOCK - 1) / BLOCK, FOLD_MAX_BLOCKS);
#define CALL_FOLD(PV)                                                                                 \
    case PV: tm.launch(particle_fold_kernel<PV>, dim3(grid), dim3(BLOCK), 0, (const float*)p.costs.p, h->core.costs.p,   \
                       mk.accumulate, mk.reset_next, h->d.N, p.mode, p.k); break;
    switch (p.P) {
        CALL_FOLD(1) CALL_FOLD(2) CALL_FOLD(3) CALL_FOLD(4) CALL_FOLD(5) CALL_FOLD(6) CALL_FOLD(7) CALL_FOLD(8)
        CALL_FOLD(9) CALL_FOLD(10) CALL_FOLD(11) CALL_FOLD(12) CALL_FOLD(13) CALL_FOLD(14) CALL_FOLD(15) CALL_FOLD(16)
    default: h->min_key.cancel_rollout(); return fail(h, MPPI_E_STATE, "no particles set");
    }
#undef CALL_FOLD
    static_assert(MPPI_MAX_PARTICLES == 16, "one instantiation of the fold per particle count");
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

// mppi_rollout_cost while particles are set (the caller has run check_ready): every sample from every particle, then the
// fold; with the control-cost term on, kappa * A_i once, behind the fold.
int rollout_particles(mppi_handle_t h, hipStream_t s) {
    auto& p = h->part;
    if (h->opt.mapping == 1) return fail(h, MPPI_E_INVALID, "particles are not available with mapping = 1");
    if (p.mode == MPPI_RISK_CVAR && (p.k < 1 || p.k > p.P))  // (before anything is launched)
        return fail(h, MPPI_E_INVALID, "risk measure: CVAR needs 1 <= k <= P (mppi_set_risk / mppi_set_particles)");
    // the map from particle to ensemble member (before anything is launched): its length is the particle count, every entry a member
    ModelCtx ctx = h->model.ctx;
    if (!p.members.empty()) {
        if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "particle members belong to the learned-dynamics models");
        if ((int)p.members.size() != p.P)
            return fail(h, MPPI_E_INVALID, "particle members: the map's length is not the particle count (mppi_set_particle_members / mppi_set_particles)");
        for (int e : p.members)
            if (e >= h->model.mlp_members)
                return fail(h, MPPI_E_INVALID, "particle members: an entry is not a member of the ensemble (mppi_set_mlp_ensemble)");
    }
    if (int rc = flush_state_seq(h, s)) return rc;  // (the particle launch does not carry the rider block)
    if (int rc = reserve_particle_costs(h, p.P)) return rc;
    if (!p.members.empty()) {  // the members' offsets into the weight buffer, staged in stream order; the launch's ctx starts at member 0
        if (!p.member_off) HIP_TRY(h, p.member_off.alloc_set(MPPI_MAX_PARTICLES, 0));
        if (!p.member_off_valid) {
            float bits[MPPI_MAX_PARTICLES] = {};  // (the int32 offsets, as the staging ring carries them)
            for (int m = 0; m < p.P; ++m) {
                const int32_t off = p.members[(size_t)m] * mlp_table_len(h);
                std::memcpy(&bits[m], &off, sizeof(off));
            }
            if (int rc = upload_small(h, reinterpret_cast<float*>(p.member_off.p), bits, MPPI_MAX_PARTICLES, s)) return rc;
            p.member_off_valid = true;
        }
        ctx.ref = h->model.mlp.p;
        ctx.pad = reinterpret_cast<const uint8_t*>(p.member_off.p);
        ctx.pad_stride = p.P;
    }
    const bool gen = regen_noise(h);
    if (!gen && !h->core.tiles_valid) return fail(h, MPPI_E_STATE, "no noise: call mppi_sample or mppi_inject_noise first");
    {
        StageTimer tm(h, 1, s);  // events on the stage's two dispatches: the start rides on the rollout, the stop on the fold
        tm.left = 2;
        const dim3 grid((unsigned)((h->d.tiles + 3) / 4), (unsigned)p.P);
#define CALL_PARTICLES(MODEL, FASTV)                                                                  \
    do {                                                                                              \
        const size_t shmem = sizeof(float) * RolloutLds::floats(h->d.R, h->d.T, h->d.row, ModelT<MODEL, FASTV>::KROW, false); \
        constexpr bool UCV = FASTV != 0;  /* the FAST kernels exist in the u_in_bounds form only (see use_fast) */ \
        constexpr bool TRK = mlp_track(MODEL);  /* (the learned models' instantiations with the tracking cost: mppi_models.hpp) */ \
        tm.launch(TRK && mlp_tracking(ctx)                                                            \
                      ? (gen ? rollout_particles_kernel<MODEL, FASTV, true, UCV, TRK> : rollout_particles_kernel<MODEL, FASTV, false, UCV, TRK>) \
                      : (gen ? rollout_particles_kernel<MODEL, FASTV, true, UCV> : rollout_particles_kernel<MODEL, FASTV, false, UCV>), \
                  grid, dim3(BLOCK), shmem, (const float4*)h->core.noise.p, (const float*)h->core.mean.p,                    \
                  (const float*)p.table.p, h->core.x0_cur, p.costs.p, h->core.mean_used.p, h->core.x0_used.p, h->d,         \
                  h->core.gen, ctx);                                                                  \
    } while (0)
        MPPI_DISPATCH(h, CALL_PARTICLES);
#undef CALL_PARTICLES
        HIP_TRY(h, hipGetLastError());
        p.costs_valid = true;
        if (int rc = fold_particles(h, tm)) return rc;
    }
    if (h->ac.on) return mppi_add_action_cost(h, h->ac.lambda, (void*)s);  // fold first, then the term
    return MPPI_OK;
}

// mppi_clone_state: the table, P, the mode, k and the last matrix (the caller has synchronised the device)
int clone_particles(mppi_handle_t dst, mppi_handle_t src) {
    auto &dp = dst->part, &sp = src->part;
    dp.P = sp.P; dp.mode = sp.mode; dp.k = sp.k; dp.costs_valid = false;
    dp.members = sp.members; dp.member_off_valid = false;  // (the offsets are staged again by dst's next rollout)
    if (sp.table) {
        if (!dp.table) HIP_TRY(dst, dp.table.alloc(sp.table.n));
        HIP_TRY(dst, hipMemcpy(dp.table.p, sp.table.p, sizeof(float) * sp.table.n, hipMemcpyDeviceToDevice));
    }
    if (sp.P > 0 && sp.costs_valid) {
        if (int rc = reserve_particle_costs(dst, sp.P)) return rc;
        HIP_TRY(dst, hipMemcpy(dp.costs.p, sp.costs.p, sizeof(float) * (size_t)sp.P * (size_t)src->d.N, hipMemcpyDeviceToDevice));
        dp.costs_valid = true;
    }
    return MPPI_OK;
}

}  // namespace mppi

extern "C" {

int mppi_set_particles(mppi_handle_t h, const float* particles, int P, int on_device, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (P < 0 || P > MPPI_MAX_PARTICLES) return fail(h, MPPI_E_INVALID, "particles: 0 <= P <= MPPI_MAX_PARTICLES (16)");
    hipStream_t s = (hipStream_t)stream;
    auto& p = h->part;
    if (int rc = flush_state_seq(h, s)) return rc;
    if (P == 0 || !particles) {  // off
        p.P = 0;
        p.costs_valid = false;
        p.members.clear();  // (the map belongs to the particles it was given for)
        p.member_off_valid = false;
        return MPPI_OK;
    }
    if (h->opt.mapping == 1) return fail(h, MPPI_E_INVALID, "particles are not available with mapping = 1");
    if (h->cfg.model != MPPI_MODEL_GENERIC) {  // (a generic handle only records P: its callables own the start states)
        const size_t n = (size_t)P * (size_t)h->ds;
        if (!on_device)
            for (size_t j = 0; j < n; ++j)
                if (!std::isfinite(particles[j])) return fail(h, MPPI_E_INVALID, "particles: every value must be finite");
        if (!p.table) HIP_TRY(h, p.table.alloc_set((size_t)MPPI_MAX_PARTICLES * (size_t)h->ds, 0));
        if (int rc = copy_small(h, p.table.p, particles, sizeof(float) * n, true, on_device != 0, s)) return rc;
    }
    if (int rc = reserve_particle_costs(h, P)) return rc;
    if (P != p.P) p.costs_valid = false;  // (the matrix of another particle count is not this one's)
    p.P = P;
    return MPPI_OK;
}

int mppi_get_particles(mppi_handle_t h, float* out, int* P_out, int on_device, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (P_out) *P_out = h->part.P;
    if (!out || h->part.P == 0) return MPPI_OK;
    if (!h->part.table) return fail(h, MPPI_E_STATE, "generic handle: it records the particle count only");
    return copy_small(h, out, h->part.table.p, sizeof(float) * (size_t)h->part.P * (size_t)h->ds, on_device != 0, true,
                      (hipStream_t)stream);
}

int mppi_set_particle_members(mppi_handle_t h, const int* members, int P) {
    if (!h) return MPPI_E_INVALID;
    auto& p = h->part;
    if (!members || P == 0) {  // none
        p.members.clear();
        p.member_off_valid = false;
        return MPPI_OK;
    }
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "particle members belong to the learned-dynamics models");
    if (P < 0 || P > MPPI_MAX_PARTICLES) return fail(h, MPPI_E_INVALID, "particle members: 0 <= P <= MPPI_MAX_PARTICLES (16)");
    for (int m = 0; m < P; ++m)
        if (members[m] < 0 || members[m] >= MPPI_MAX_PARTICLES)
            return fail(h, MPPI_E_INVALID, "particle members: every entry is a member index, 0 <= e < MPPI_MAX_PARTICLES (16)");
    p.members.assign(members, members + P);  // (checked against P and the ensemble where the rollout is launched)
    p.member_off_valid = false;
    return MPPI_OK;
}

int mppi_get_particle_members(mppi_handle_t h, int* out, int* P_out) {
    if (!h) return MPPI_E_INVALID;
    if (P_out) *P_out = (int)h->part.members.size();
    if (out) std::copy(h->part.members.begin(), h->part.members.end(), out);
    return MPPI_OK;
}

int mppi_set_risk(mppi_handle_t h, int mode, int k) {
    if (!h) return MPPI_E_INVALID;
    if (mode < MPPI_RISK_MEAN || mode > MPPI_RISK_CVAR) return fail(h, MPPI_E_INVALID, "risk measure: MPPI_RISK_MEAN, _WORST or _CVAR");
    h->part.mode = mode;
    h->part.k = k;  // (checked against P where the fold is launched: either call may come first)
    return MPPI_OK;
}

int mppi_get_risk(mppi_handle_t h, int* mode_out, int* k_out) {
    if (!h) return MPPI_E_INVALID;
    if (mode_out) *mode_out = h->part.mode;
    if (k_out) *k_out = h->part.k;
    return MPPI_OK;
}

int mppi_get_particle_costs(mppi_handle_t h, float* out, int on_device, void* stream) {
    if (!h || !out) return fail(h, MPPI_E_INVALID, "null");
    const auto& p = h->part;
    if (p.P == 0 || !p.costs_valid) return fail(h, MPPI_E_STATE, "no particle costs: set particles and roll out (or mppi_set_particle_costs) first");
    return copy_small(h, out, p.costs.p, sizeof(float) * (size_t)p.P * (size_t)h->d.N, on_device != 0, true, (hipStream_t)stream);
}

int mppi_set_particle_costs(mppi_handle_t h, const float* src, int on_device, void* stream) {
    if (!h || !src) return fail(h, MPPI_E_INVALID, "null");
    auto& p = h->part;
    if (p.P == 0) return fail(h, MPPI_E_STATE, "no particles set: call mppi_set_particles first");
    if (p.mode == MPPI_RISK_CVAR && (p.k < 1 || p.k > p.P))  // (before the matrix is touched)
        return fail(h, MPPI_E_INVALID, "risk measure: CVAR needs 1 <= k <= P (mppi_set_risk / mppi_set_particles)");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = reserve_particle_costs(h, p.P)) return rc;
    if (int rc = copy_small(h, p.costs.p, src, sizeof(float) * (size_t)p.P * (size_t)h->d.N, true, on_device != 0, s)) return rc;
    p.costs_valid = true;
    StageTimer untimed(h, -1, s);
    return fold_particles(h, untimed);
}

}  // extern "C"
