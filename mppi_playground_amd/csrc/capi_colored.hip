// capi_colored.hip — C ABI (include/mppi_hip.h): temporally correlated (AR(1)) sampling noise — the setting, its per-column
// table and the launches of the filtered draws (sample_colored_kernel, posterior_colored_kernel: mppi_sample.hpp).
#include "mppi_handle.hpp"
#include "mppi_sample.hpp"

namespace mppi {

// the carry width the kernels are compiled for: dim_control itself up to 4 (registers), 0 for every wider row (read back)
#define MPPI_DISPATCH_COLORED(dc, CALL)                                                               \
    switch (dc) {                                                                                     \
    case 1: CALL(1); break;                                                                           \
    case 2: CALL(2); break;                                                                           \
    case 3: CALL(3); break;                                                                           \
    case 4: CALL(4); break;                                                                           \
    default: CALL(0); break;                                                                          \
    }

int sample_colored(mppi_handle_t h, StageTimer& tm) {
    const unsigned grid = (unsigned)((h->d.tiles + 3) / 4);
#define CALL_SAMPLE(DC)                                                                               \
    tm.launch(sample_colored_kernel<DC>, dim3(grid), dim3(BLOCK), 0, (float4*)h->core.noise, h->d, h->core.gen, (const float*)sigma_table(h), \
              (const float*)h->color.tab)
    MPPI_DISPATCH_COLORED(h->dc, CALL_SAMPLE);
#undef CALL_SAMPLE
    return MPPI_OK;
}

int posterior_colored(mppi_handle_t h, const GenCtx& g, const float* loc_dev, int k, float* samples_out_dev, hipStream_t s) {
    const unsigned grid = (unsigned)((k + BLOCK - 1) / BLOCK);
#define CALL_POSTERIOR(DC)                                                                            \
    hipLaunchKernelGGL(posterior_colored_kernel<DC>, dim3(grid), dim3(BLOCK), 0, s, loc_dev, k, samples_out_dev, h->d, g,  \
                       (const float*)sigma_table(h), (const float*)h->color.tab)
    MPPI_DISPATCH_COLORED(h->dc, CALL_POSTERIOR);
#undef CALL_POSTERIOR
    return MPPI_OK;
}

}  // namespace mppi

extern "C" {

int mppi_set_noise_correlation(mppi_handle_t h, const float* beta_host) {
    if (!h) return MPPI_E_INVALID;
    if (!h->limits_set) return fail(h, MPPI_E_STATE, "dim_control > 4: call mppi_set_control_limits first");
    bool any = false;
    for (int k = 0; beta_host && k < h->dc; ++k) {
        if (!(beta_host[k] >= 0.0f && beta_host[k] < 1.0f))
            return fail(h, MPPI_E_INVALID, "noise correlation: need 0 <= beta < 1 in every control dimension");
        any = any || beta_host[k] > 0.0f;
    }
    auto& c = h->color;
    c.beta.assign((size_t)h->dc, 0.0f);
    if (any) {
        const size_t C = 4 * (size_t)h->d.R;
        std::vector<float> tab(2 * C, 0.0f);
        for (int k = 0; k < h->dc; ++k) c.beta[k] = beta_host[k];
        for (int f = 0; f < h->d.row; ++f) {
            tab[f] = c.beta[f % h->dc];
            tab[C + f] = colored_alpha(c.beta[f % h->dc]);
        }
        if (!c.tab) HIP_TRY(h, c.tab.alloc(2 * C));
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, hipMemcpy(c.tab, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    }
    c.on = any;
    h->core.tiles_valid = h->core.tiles_valid && h->core.injected;  // (tiles drawn under the old setting are stale)
    return MPPI_OK;
}

int mppi_get_noise_correlation(mppi_handle_t h, float* beta_out_host) {
    if (!h || !beta_out_host) return fail(h, MPPI_E_INVALID, "null");
    for (int k = 0; k < h->dc; ++k) beta_out_host[k] = h->color.beta.empty() ? 0.0f : h->color.beta[k];
    return MPPI_OK;
}

}  // extern "C"
