// capi_topk.hip — C ABI (include/mppi_hip.h): queries after a solve — posterior draws, weights, re-rolled actions and
// samples, get_top_samples and its sharded halves.
#include "mppi_handle.hpp"
#include "mppi_topk.hpp"

namespace mppi {

// the select state (kept zeroed between calls) and the candidate buffer; mppi_create, set-up path
int topk_alloc(mppi_handle_t h) {
    HIP_TRY(h, h->topk.hist.alloc_set(3 * TOPK_BINS + 2, 0));
    HIP_TRY(h, h->topk.sel.alloc(3));
    HIP_TRY(h, h->topk.cand.alloc(TOPK_MAX));
    return MPPI_OK;
}

// candidate buffer for k words, padded to a power of two (the large-k sort works on 2^m words)
static int topk_reserve(mppi_handle_t h, int k) {
    size_t need = TOPK_MAX;
    while (need < (size_t)k) need <<= 1;
    if (need <= h->topk.cand.n) return MPPI_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, h->topk.cand.alloc(need));
    return MPPI_OK;
}

// radix select of this handle's k smallest costs -> h->topk.cand (unordered, global indices)
static int topk_select(mppi_handle_t h, int k, hipStream_t s) {
    if (k < 1 || k > h->d.N) return fail(h, MPPI_E_INVALID, "top samples: need 1 <= k <= num_samples");
    if (h->d.sample_offset + h->d.N >= ((int64_t)1 << 32)) return fail(h, MPPI_E_INVALID, "top samples: global sample indices must be < 2^32");
    if (int rc = topk_reserve(h, k)) return rc;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((h->d.N + BLOCK * 8 - 1) / (BLOCK * 8), 1024));
    unsigned* hist = h->topk.hist;
    unsigned* counters = h->topk.hist + 3 * TOPK_BINS;
    hipLaunchKernelGGL(topk_hist_kernel<0>, dim3(grid), dim3(BLOCK), 0, s, h->core.costs, h->d.N, (unsigned)k, hist, h->topk.sel);
    hipLaunchKernelGGL(topk_hist_kernel<1>, dim3(grid), dim3(BLOCK), 0, s, h->core.costs, h->d.N, (unsigned)k, hist, h->topk.sel);
    hipLaunchKernelGGL(topk_hist_kernel<2>, dim3(grid), dim3(BLOCK), 0, s, h->core.costs, h->d.N, (unsigned)k, hist, h->topk.sel);
    hipLaunchKernelGGL(topk_collect_kernel, dim3(grid), dim3(BLOCK), 0, s, h->core.costs, h->d.N, (unsigned)k, h->d.sample_offset,
                       hist, h->topk.sel, h->topk.cand, counters);
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

// ascending sort of the k > TOPK_MAX candidate words at h->topk.cand (see topk_sort_local_kernel)
static int topk_sort_large(mppi_handle_t h, int k, hipStream_t s) {
    int P = TOPK_MAX;
    while (P < k) P <<= 1;
    if (P > k) hipLaunchKernelGGL(topk_pad_kernel, dim3((unsigned)((P - k + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, h->topk.cand, k, P);
    hipLaunchKernelGGL(topk_sort_local_kernel<true>, dim3((unsigned)(P / TOPK_MAX)), dim3(TOPK_MAX), 0, s, h->topk.cand, 0);
    for (int size = 2 * TOPK_MAX; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride >= TOPK_MAX; stride >>= 1)
            hipLaunchKernelGGL(topk_sort_global_kernel, dim3((unsigned)((P / 2 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, h->topk.cand,
                               P, size, stride);
        hipLaunchKernelGGL(topk_sort_local_kernel<false>, dim3((unsigned)(P / TOPK_MAX)), dim3(TOPK_MAX), 0, s, h->topk.cand, size);
    }
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

// A launch whose dynamic LDS grows with the length of a control row (T * dim_control): beyond 32 KiB it is held against the
// kernel's own static LDS and the 64 KiB a block gets without opting in, so that a horizon too long for the staging fails
// with a message instead of a bare launch error.  Queried only in that rare case.
static int check_row_lds(mppi_handle_t h, const void* kernel, size_t dyn, const char* what) {
    if (dyn <= 32 * 1024) return MPPI_OK;
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, kernel) != hipSuccess) { (void)hipGetLastError(); return MPPI_OK; }
    if (fa.sharedSizeBytes + dyn > 64 * 1024)
        return fail(h, MPPI_E_INVALID, std::string(what) + ": control rows of T * dim_control = " + std::to_string(h->d.row) +
                    " floats need " + std::to_string((fa.sharedSizeBytes + dyn + 1023) / 1024) + " KiB of LDS per block (limit 64 KiB): "
                    "horizon x dim_control too long for this query");
    return MPPI_OK;
}

// sort k candidates, weigh and re-roll them; `clean` also resets the select state (after topk_select).  `cand` is
// h->topk.cand when k > TOPK_MAX (sorted in place).
static int topk_rollout(mppi_handle_t h, const unsigned long long* cand, int k, float lambda, float* states_out,
                        float* weights_out, bool clean, bool need_local, hipStream_t s, bool direct = false) {
    const bool gen = regen_noise(h);  // (every caller has refused generic handles, the only wide ones: check_ready)
    if (!gen && !h->core.tiles_valid) return fail(h, MPPI_E_STATE, "no noise: solve first");
    if (!gen && !need_local)
        return fail(h, MPPI_E_STATE, "candidates of other shards can only be re-rolled from regenerated noise (noise_regen = 1, no injection)");
    unsigned* hist = clean ? h->topk.hist : nullptr;
    unsigned* counters = clean ? h->topk.hist + 3 * TOPK_BINS : nullptr;
    if (k <= TOPK_MAX) {
#define CALL_TOPK(MODEL, FASTV)                                                                       \
    if (int rc = check_row_lds(h, (const void*)topk_rollout_kernel<MODEL, FASTV, false>, sizeof(float) * TopkLds::floats(h->d.R, false, gen), "get_top_samples")) return rc; \
    hipLaunchKernelGGL((topk_rollout_kernel<MODEL, FASTV, false>), dim3((unsigned)((k + WAVE - 1) / WAVE)), dim3(TOPK_MAX), sizeof(float) * TopkLds::floats(h->d.R, false, gen), s, cand, k, \
                       direct ? (const float*)h->core.costs : (const float*)nullptr, direct ? (int)h->d.N : 0, h->core.noise, gen,  \
                       h->core.mean_used, h->core.x0_used, h->reduce.solve_stats, lambda, states_out, weights_out, hist, counters,  \
                       h->d, h->core.gen, h->model.ctx)
        MPPI_DISPATCH(h, CALL_TOPK);
#undef CALL_TOPK
    } else {
        if (int rc = topk_sort_large(h, k, s)) return rc;
        const unsigned grid = (unsigned)((k + WAVE - 1) / WAVE);
#define CALL_TOPK_SORTED(MODEL, FASTV)                                                                \
    if (int rc = check_row_lds(h, (const void*)topk_rollout_kernel<MODEL, FASTV, true>, sizeof(float) * TopkLds::floats(h->d.R, true, gen), "get_top_samples")) return rc; \
    hipLaunchKernelGGL((topk_rollout_kernel<MODEL, FASTV, true>), dim3(grid), dim3(WAVE), sizeof(float) * TopkLds::floats(h->d.R, true, gen), s, (const unsigned long long*)h->topk.cand, \
                       k, (const float*)nullptr, 0, h->core.noise, gen, h->core.mean_used, h->core.x0_used, h->reduce.solve_stats, lambda, states_out,  \
                       weights_out, hist, counters, h->d, h->core.gen, h->model.ctx)
        MPPI_DISPATCH(h, CALL_TOPK_SORTED);
#undef CALL_TOPK_SORTED
    }
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

}  // namespace mppi

extern "C" {

// get_samples_from_posterior, the sampling half (mppi.py:489-503): k unclamped action sequences
// loc + eps, eps ~ N(0, diag(sigma^2)) from the Philox stream of the RESERVED solve index `solve_idx` (callers advance
// their solve counter: the draw consumes the stream like the reference's global generator).  Roll them out with
// mppi_rollout_actions(x0_dev = the posterior's state).
int mppi_sample_posterior(mppi_handle_t h, uint32_t solve_idx, const float* loc_dev, int k, float* samples_out_dev,
                          void* stream) {
    if (!h || !loc_dev || !samples_out_dev || k < 1) return fail(h, MPPI_E_INVALID, "bad sample_posterior arguments");
    if (!h->limits_set) return fail(h, MPPI_E_STATE, "dim_control > 4: call mppi_set_control_limits first");
    const GenCtx g{h->core.gen.seed_lo, h->core.gen.seed_hi, solve_idx};
    const unsigned grid = (unsigned)(((int64_t)k * h->d.R + BLOCK - 1) / BLOCK);
    if (h->color.on) {  // the filter of the solves' draw (`_noise_distribution` is what the posterior follows)
        if (int rc = posterior_colored(h, g, loc_dev, k, samples_out_dev, (hipStream_t)stream)) return rc;
    } else if (h->wide || h->cov.on)  // sigma per column: the table the solves draw from (mppi.py:416-418: `_noise_distribution` follows the covariance)
        hipLaunchKernelGGL(posterior_sample_kernel<true>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, loc_dev, k,
                           samples_out_dev, h->d, g, (const float*)sigma_table(h));
    else
        hipLaunchKernelGGL(posterior_sample_kernel<false>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, loc_dev, k,
                           samples_out_dev, h->d, g, (const float*)nullptr);
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

int mppi_weights(mppi_handle_t h, float lambda, float cmin, float sum_e, float* w_out, void* stream) {
    if (!h || !w_out || !(lambda > 0.0f)) return fail(h, MPPI_E_INVALID, "bad weights arguments");
    const unsigned grid = (unsigned)((h->d.N + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(weights_kernel, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, h->core.costs, h->d.N, lambda, cmin,
                       sum_e, w_out);
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

int mppi_rollout_actions(mppi_handle_t h, const float* actions_dev, int k, const float* x0_dev, float* states_out,
                         void* stream) {
    if (!h || !actions_dev || !states_out || k < 1) return fail(h, MPPI_E_INVALID, "bad rollout_actions arguments");
    if (int rc = check_ready(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const float* x0 = x0_dev ? x0_dev : h->core.x0_cur;  // an explicit start state leaves the solver's own untouched
    const unsigned grid = (unsigned)((k + WAVE - 1) / WAVE);
#define CALL_RA(MODEL, FASTV)                                                                         \
    hipLaunchKernelGGL((rollout_actions_kernel<MODEL, FASTV>), dim3(grid), dim3(WAVE), 0, s, actions_dev, k, h->d.T, \
                       x0, states_out, h->model.ctx)
    MPPI_DISPATCH(h, CALL_RA);
#undef CALL_RA
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

int mppi_rollout_samples(mppi_handle_t h, const int64_t* idx_dev, int k, float* states_out, void* stream) {
    if (!h || !idx_dev || !states_out || k < 1) return fail(h, MPPI_E_INVALID, "bad rollout_samples arguments");
    if (int rc = check_ready(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = need_tiles(h, s)) return rc;
    const unsigned grid = (unsigned)((k + WAVE - 1) / WAVE);
#define CALL_RS(MODEL, FASTV)                                                                         \
    hipLaunchKernelGGL((rollout_samples_kernel<MODEL, FASTV>), dim3(grid), dim3(WAVE), 0, s, h->core.noise, h->core.mean_used, \
                       idx_dev, k, h->core.x0_used, states_out, h->d, h->model.ctx)
    MPPI_DISPATCH(h, CALL_RS);
#undef CALL_RS
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

int mppi_top_samples(mppi_handle_t h, int k, float lambda, float* states_out, float* weights_out, void* stream) {
    if (!h || !states_out || !weights_out || !(lambda > 0.0f || lambda == MPPI_LAMBDA_DEVICE))
        return fail(h, MPPI_E_INVALID, "bad top_samples arguments");
    if (int rc = check_ready(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (h->d.N <= TOPK_DIRECT_MAX && k <= TOPK_MAX) {  // small problems (the reference examples' sizes): ONE launch
        if (k < 1 || k > h->d.N) return fail(h, MPPI_E_INVALID, "top samples: need 1 <= k <= num_samples");
        if (h->d.sample_offset + h->d.N >= ((int64_t)1 << 32)) return fail(h, MPPI_E_INVALID, "top samples: global sample indices must be < 2^32");
        return topk_rollout(h, nullptr, k, lambda, states_out, weights_out, false, true, s, true);
    }
    if (int rc = topk_select(h, k, s)) return rc;
    return topk_rollout(h, h->topk.cand, k, lambda, states_out, weights_out, true, true, s);
}

int mppi_top_candidates(mppi_handle_t h, int k, uint64_t* cand_out_dev, void* stream) {
    if (!h || !cand_out_dev) return fail(h, MPPI_E_INVALID, "bad top_candidates arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = topk_select(h, k, s)) return rc;
    HIP_TRY(h, hipMemcpyAsync(cand_out_dev, h->topk.cand, sizeof(uint64_t) * (size_t)k, hipMemcpyDeviceToDevice, s));
    // leave the select state clean for the next call
    HIP_TRY(h, hipMemsetAsync(h->topk.hist, 0, sizeof(unsigned) * (3 * TOPK_BINS + 2), s));
    return MPPI_OK;
}

int mppi_rollout_candidates(mppi_handle_t h, const uint64_t* cand_dev, int k, float lambda, float* states_out,
                            float* weights_out, void* stream) {
    if (!h || !cand_dev || !states_out || !weights_out || !(lambda > 0.0f || lambda == MPPI_LAMBDA_DEVICE) || k < 1)
        return fail(h, MPPI_E_INVALID, "bad rollout_candidates arguments");
    if (int rc = check_ready(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (k > TOPK_MAX) {  // the large-k sort works in place on the handle's padded buffer
        if (int rc = topk_reserve(h, k)) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->topk.cand, cand_dev, sizeof(uint64_t) * (size_t)k, hipMemcpyDeviceToDevice, s));
        return topk_rollout(h, h->topk.cand, k, lambda, states_out, weights_out, false, false, s);
    }
    return topk_rollout(h, reinterpret_cast<const unsigned long long*>(cand_dev), k, lambda, states_out, weights_out, false,
                        false, s);
}

}  // extern "C"
