// capi_covariance.hip — C ABI (include/mppi_hip.h): covariance adaptation of the sampling noise (the sketch at
// mppi.py:400-418) — its settings, the per-step sigma table and the step that runs after the weights of a solve.
#include <cmath>

#include "mppi_handle.hpp"
#include "mppi_variance.hpp"

namespace mppi {

// buffers of the step, allocated when the adaptation is first switched on (set-up path)
int cov_alloc(mppi_handle_t h) {
    auto& c = h->cov;
    if (!c.lim) HIP_TRY(h, c.lim.alloc(2 * (size_t)h->dc));
    if (!c.part) HIP_TRY(h, c.part.alloc((size_t)REDUCE_MAX_BLOCKS * h->reduce.colsp));
    if (!c.live) HIP_TRY(h, c.live.alloc_set(REDUCE_MAX_BLOCKS, 0));
    return MPPI_OK;
}

// table[f] = sigmas[f % n] over the row, zeros past it (blocking; wide handles fill theirs in mppi_set_control_limits)
int fill_sigma_table(mppi_handle_t h, const float* sigmas, int n) {
    if (h->wide) return MPPI_OK;
    std::vector<float> tab(4 * (size_t)h->d.R, 0.0f);
    for (int f = 0; f < h->d.row; ++f) tab[f] = sigmas[f % n];
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(h->cov.sigtab, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    return MPPI_OK;
}

}  // namespace mppi

extern "C" {

int mppi_set_covariance_adaptation(mppi_handle_t h, int enable, float rate, float floor, const float* sigma_min_host,
                                   const float* sigma_max_host) {
    if (!h) return MPPI_E_INVALID;
    if (!(rate >= 0.0f && rate <= 1.0f)) return fail(h, MPPI_E_INVALID, "covariance adaptation: rate must lie in [0, 1]");
    if (!(floor >= 0.0f) || !std::isfinite(floor)) return fail(h, MPPI_E_INVALID, "covariance adaptation: floor must be >= 0");
    if (enable && (h->xchg.p2p_enabled || h->xchg.comm_enabled))
        return fail(h, MPPI_E_INVALID, "covariance adaptation is not available for sharded solves (the variance would need a second exchange)");
    if (enable && !h->limits_set) return fail(h, MPPI_E_STATE, "dim_control > 4: call mppi_set_control_limits first");
    std::vector<float> lim(2 * (size_t)h->dc);
    for (int k = 0; k < h->dc; ++k) {
        lim[k] = sigma_min_host ? sigma_min_host[k] : 0.0f;
        lim[h->dc + k] = sigma_max_host ? sigma_max_host[k] : INFINITY;
        if (!(lim[k] >= 0.0f) || !(lim[k] <= lim[h->dc + k]))
            return fail(h, MPPI_E_INVALID, "covariance adaptation: need 0 <= sigma_min <= sigma_max");
    }
    if (enable) {  // (switching off allocates nothing; the step's buffers exist from the first time it is switched on)
        if (int rc = cov_alloc(h)) return rc;
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, hipMemcpy(h->cov.lim, lim.data(), sizeof(float) * lim.size(), hipMemcpyHostToDevice));
    }
    h->cov.on = enable != 0;
    h->cov.rate = rate;
    h->cov.floor = floor;
    h->cov.ready = false;
    return MPPI_OK;
}

int mppi_update_covariance(mppi_handle_t h, float lambda, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (!h->cov.on) return fail(h, MPPI_E_STATE, "covariance adaptation is off (mppi_set_covariance_adaptation)");
    if (!h->cov.ready || !h->reduce.summary_valid)
        return fail(h, MPPI_E_STATE, "mppi_update_covariance belongs between mppi_weights_reduce and mppi_finalize");
    if (!h->core.tiles_valid) return fail(h, MPPI_E_STATE, "no noise: call mppi_sample or mppi_inject_noise first");
    const float* lam_dev = nullptr;
    if (int rc = resolve_lambda(h, lambda, &lam_dev)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = h->reduce.last_reduce_blocks;  // the reduction's own split of the tiles
    const dim3 grid((unsigned)blocks, (unsigned)h->reduce.nchunks);
    hipLaunchKernelGGL(weighted_variance_kernel, grid, dim3(BLOCK), 0, s, h->core.noise, h->core.mean, h->core.costs,
                       h->min_key.cur(), h->reduce.summary, h->wide ? (const float*)h->core.coltab : (const float*)nullptr,
                       h->cov.part, h->cov.live, h->d, lambda, lam_dev);
    hipLaunchKernelGGL(sigma_update_kernel, dim3(1), dim3(SU_BLOCK), 0, s, h->cov.part, h->cov.live, blocks, h->reduce.colsp,
                       h->d.row, h->dc, h->reduce.summary, h->cov.lim, h->cov.rate, h->cov.floor, sigma_table(h));
    HIP_TRY(h, hipGetLastError());
    h->cov.ready = false;
    return MPPI_OK;
}

int mppi_get_sigma_table(mppi_handle_t h, float* out, int on_device, void* stream) {
    if (!h || !out) return fail(h, MPPI_E_INVALID, "null");
    if (!h->limits_set) return fail(h, MPPI_E_STATE, "dim_control > 4: call mppi_set_control_limits first");
    return copy_small(h, out, sigma_table(h), sizeof(float) * (size_t)h->d.row, on_device != 0, true, (hipStream_t)stream);
}

int mppi_set_sigma_table(mppi_handle_t h, const float* table, int on_device, void* stream) {
    if (!h || !table) return fail(h, MPPI_E_INVALID, "null");
    if (!h->limits_set) return fail(h, MPPI_E_STATE, "dim_control > 4: call mppi_set_control_limits first");
    return copy_small(h, sigma_table(h), table, sizeof(float) * (size_t)h->d.row, true, on_device != 0, (hipStream_t)stream);
}

}  // extern "C"
