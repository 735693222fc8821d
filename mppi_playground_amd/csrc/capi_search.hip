// capi_search.hip — C ABI (include/mppi_hip.h): the temperature — softmax statistics, the ESSPS / LBPS searches (host loops
// and device-resident chains, Brent in one launch) and the MPO dual.
#include "mppi_handle.hpp"

namespace mppi {

__global__ __launch_bounds__(BLOCK) void stats_partial_kernel(const float* __restrict__ costs, int64_t N,
                                                             const unsigned* __restrict__ min_key, float lambda_arg,
                                                             const float* __restrict__ lambda_dev /* nullable */,
                                                             float* __restrict__ part /*[STATS_BLOCKS][4]*/) {
    __shared__ float s_p[BLOCK / WAVE][4];
    const float lambda = lambda_dev ? *lambda_dev : lambda_arg;
    const float cmin = key_to_float(*min_key);
    const float xmax = (-cmin) / lambda;
    float se, se2, sec, cmax;
    stats_partial_thread([&](int64_t i, int) { return costs[i]; }, N, (int64_t)blockIdx.x * BLOCK + threadIdx.x,
                         (int64_t)gridDim.x * BLOCK, lambda, xmax, se, se2, sec, cmax);
    stats_partial_wave(se, se2, sec, cmax);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { s_p[wid][0] = se; s_p[wid][1] = se2; s_p[wid][2] = sec; s_p[wid][3] = cmax; }
    __syncthreads();
    if (threadIdx.x < 4) part[blockIdx.x * 4 + threadIdx.x] = stats_partial_fold(s_p, threadIdx.x);
}

__global__ __launch_bounds__(WAVE) void stats_combine_kernel(const float* __restrict__ part, int nblocks,
                                                            const unsigned* __restrict__ min_key,
                                                            double* __restrict__ out /*[5] mapped host*/) {
    double se, se2, sec;
    float cmax;
    stats_combine_wave([&](int b, int j) { return part[b * 4 + j]; }, nblocks, (int)threadIdx.x, se, se2, sec, cmax);
    if (threadIdx.x == 0) {
        out[0] = (double)key_to_float(*min_key); out[1] = (double)cmax; out[2] = se; out[3] = se2; out[4] = sec;
    }
}

__global__ __launch_bounds__(STATS_THREADS) void stats_multi_kernel(const float* __restrict__ costs, int64_t N,
                                                                    const unsigned* __restrict__ min_key,
                                                                    const float* __restrict__ lams,
                                                                    float* __restrict__ part,
                                                                    float* __restrict__ part_max /* nullable: [blocks] max c */) {
    __shared__ StatsLds lds;
    const float v = stats_multi_block(costs, N, key_to_float(*min_key), lams, part_max, lds);
    if (threadIdx.x < STATS_L * 3) part[(int64_t)blockIdx.x * STATS_L * 3 + threadIdx.x] = v;
}

__global__ __launch_bounds__(1024) void stats_multi_combine_kernel(const float* __restrict__ part, int nblocks,
                                                                   double* __restrict__ out /*[STATS_L][3] mapped*/) {
    __shared__ double s_acc[STATS_COMB_GROUPS * STATS_L * 3];
    stats_combine_columns(part, nblocks, s_acc, out);
}

__global__ __launch_bounds__(1024) void essps_select_kernel(const float* __restrict__ part, int nblocks, double target_ess,
                                                            mppi::host::EsspsRange range, EsspsDev* __restrict__ st,
                                                            float* __restrict__ lams, float* __restrict__ lams0,
                                                            float* __restrict__ lambda_out,
                                                            double* __restrict__ lambda_host) {
    __shared__ double s_acc[STATS_COMB_GROUPS * STATS_L * 3];
    __shared__ double s_sum[STATS_L * 3];
    __shared__ double s_ess[STATS_L], s_grid[STATS_L], s_lgrid[STATS_L];
    stats_combine_columns(part, nblocks, s_acc, s_sum);
    if (threadIdx.x >= WAVE) return;  // the scalar step: one wave, lane j owns temperature j where that helps
    essps_select_step<0>(s_sum, s_ess, s_grid, s_lgrid, target_ess, range, st, lams, lams0, lambda_out, lambda_host,
                         (int)threadIdx.x);
}

__global__ __launch_bounds__(BRENT_THREADS) void lbps_brent_kernel(const float* __restrict__ costs, int64_t N,
                                                                   const unsigned* __restrict__ min_key, int nvb, int per_thread,
                                                                   double delta, double lam_min, double lam_max, BrentCtx bx,
                                                                   float* __restrict__ lambda_out,
                                                                   double* __restrict__ lambda_host /*[3]: next, used, probes*/) {
    extern __shared__ float s_cost[];  // BrentStageLds: [per_thread][blockDim.x] when staged
    __shared__ BrentLds L;
    const int tid = threadIdx.x;
    const bool staged = per_thread <= BRENT_STAGE_MAX;
    const long long t0 = wall_clock64();
    if (staged) {
        const int vb = (int)blockIdx.x + BRENT_LANES * (tid >> 8);
        int m = 0;
        if (vb < nvb)
            for (int64_t i = (int64_t)vb * BLOCK + (tid & (BLOCK - 1)); i < N; i += (int64_t)nvb * BLOCK, ++m)
                s_cost[m * (int)blockDim.x + tid] = costs[i];  // (read back by the same thread only: no barrier needed)
    }
    if (tid == 0) {
        L.go = 0;
#ifdef MPPI_BRENT_TRACE
        L.tlast = wall_clock64();
        for (int k = 0; k < 8; ++k) L.trace[k] = 0;
#endif
    }
    const float cmin = key_to_float(*min_key);
    __syncthreads();
    if (tid < WAVE) {  // wave 0: the search itself (every lane the same scalars); the probe's barriers pair with the loop below
        unsigned probe = 0;
        double lam = 0.0;
        int nfev = 0;
        float cmax_all = -INFINITY;  // (gathered with the first probe)
        const bool ok = mppi::host::lbps_lambda(
            [&](double x, mppi::host::SoftmaxStats& st) {
                if (tid == 0) { L.lam = (float)x; L.xmax = (-cmin) / (float)x; L.go = 1; }
                ++probe;
                BRENT_TRACE(6);  // objective + Brent step
                __syncthreads();  // (A) the other waves pick the temperature up
                BRENT_TRACE(0);  // barrier A
                brent_partials_block(costs, s_cost, staged, N, nvb, bx, probe, L);
                BRENT_TRACE(3);  // barrier B
                double se, se2, sec;
                float cmax;
                if (!brent_gather_wave(nvb, bx, probe, L, t0, se, se2, sec, cmax)) return false;
                if (probe == 1) cmax_all = cmax;
                st = mppi::host::SoftmaxStats{(double)cmin, (double)cmax_all, se, se2, sec};
                return true;
            },
            delta, lam_min, lam_max, lam, &nfev);
        if (tid == 0) L.go = 0;
        __syncthreads();  // (A) releases the other waves for good
        if (blockIdx.x == 0 && tid == 0) {
            if (!ok) { lam = NAN; *bx.error = 1; }
            *lambda_out = (float)lam;
            lambda_host[0] = lam; lambda_host[1] = lam; lambda_host[2] = (double)nfev;
#ifdef MPPI_BRENT_TRACE
            BRENT_TRACE(7);
            for (int k = 0; k < 8; ++k) bx.error[1 + k] = L.trace[k];
#endif
        }
    } else {
        unsigned probe = 0;
        for (;;) {
            __syncthreads();  // (A)
            if (!L.go) break;
            ++probe;
            brent_partials_block(costs, s_cost, staged, N, nvb, bx, probe, L);
        }
    }
}

// MPO without leaving the device (mppi.py:191-200,387-398): the dual variable and its Adam moments live in device
// memory; after the solve's weights one statistics pass at T = softplus(log T) (stats_partial_kernel reading T from
// `temp_dev`) and this one-thread step (host_search.hpp: mpo_step — the arithmetic the CPU tests pin to the reference)
// leave lambda = exp(log T) for the NEXT solve in `lambda_out`.
__global__ __launch_bounds__(WAVE) void mpo_step_kernel(const float* __restrict__ part, int nblocks,
                                                        const unsigned* __restrict__ min_key,
                                                        mppi::host::MpoState* __restrict__ st,
                                                        float* __restrict__ lambda_out, float* __restrict__ temp_dev,
                                                        double* __restrict__ lambda_host /*[2]: next, used*/) {
    double se = 0.0, se2 = 0.0, sec = 0.0;
    float cmax = -INFINITY;
    for (int b = threadIdx.x; b < nblocks; b += WAVE) {
        se += part[b * 4]; se2 += part[b * 4 + 1]; sec += part[b * 4 + 2];
        cmax = fmaxf(cmax, part[b * 4 + 3]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        se += __shfl_xor(se, m); se2 += __shfl_xor(se2, m); sec += __shfl_xor(sec, m);
        cmax = fmaxf(cmax, __shfl_xor(cmax, m));
    }
    if (threadIdx.x == 0) {
        mppi::host::MpoState s = *st;
        const double used = (double)*lambda_out;
        const mppi::host::SoftmaxStats ss{(double)key_to_float(*min_key), (double)cmax, se, se2, sec};
        const double lam = mppi::host::mpo_step(s, ss);
        *st = s;
        *lambda_out = (float)lam;
        *temp_dev = s.temperature();
        lambda_host[0] = lam; lambda_host[1] = used;
    }
}

// Grid of a statistics pass: the 32-temperature one (STATS_THREADS) or the single-temperature one (BLOCK) — also the Brent
// search's virtual blocks: its bit-equality with the host search rests on this being the number mppi_softmax_stats uses.
static int stats_blocks(mppi_handle_t h, int threads = STATS_THREADS) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(STATS_BLOCKS, (h->d.N + threads - 1) / threads));
}

// One checker per rule (`ptrs`: the handle and the call's output pointers are there).
static int check_essps(mppi_handle_t h, bool ptrs, double target_ess, double lam_min, double lam_max) {
    const bool ok = ptrs && lam_min > 0.0 && lam_max > lam_min && target_ess > 0.0;  // (false for a NaN)
    return ok ? MPPI_OK : fail(h, MPPI_E_INVALID, "bad essps arguments");
}
static int check_lbps(mppi_handle_t h, bool ptrs, double delta, double lam_min, double lam_max) {
    const bool ok = ptrs && lam_min > 0.0 && lam_max > lam_min && delta > 0.0 && delta < 1.0;  // (false for a NaN)
    return ok ? MPPI_OK : fail(h, MPPI_E_INVALID, "bad lbps arguments");
}

// The state of the device-resident ESSPS search for [lam_min, lam_max]: a cold (geometric) first grid; after that every
// finished search leaves the first grid of the next one behind (host_search.hpp: essps_first_grid).  Set-up path, blocking.
int essps_prepare(mppi_handle_t h, double lam_min, double lam_max) {
    if (h->search.essps_lo == lam_min && h->search.essps_hi == lam_max) return MPPI_OK;
    EsspsDev st{};
    float lamf[STATS_L];
    h->search.essps_range = mppi::host::essps_range(lam_min, lam_max);
    mppi::host::essps_first_grid<STATS_L>(false, 0.0, h->search.essps_range, st.grid0, st.lgrid0);
    for (int j = 0; j < STATS_L; ++j) { lamf[j] = (float)st.grid0[j]; st.grid1[j] = st.grid0[j]; st.lgrid1[j] = st.lgrid0[j]; }
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(h->search.lams_dev + STATS_L, lamf, sizeof(lamf), hipMemcpyHostToDevice));
    // (round 1's grid is rewritten by every search; a valid one for the searches that end after round 0)
    HIP_TRY(h, hipMemcpy(h->search.lams_dev + 2 * STATS_L, lamf, sizeof(lamf), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->search.essps_dev, &st, sizeof(st), hipMemcpyHostToDevice));
    h->search.essps_lo = lam_min; h->search.essps_hi = lam_max;
    return MPPI_OK;
}

int mpo_upload(mppi_handle_t h, double lambda0, double epsilon, double lr, bool lambda_too) {
    mppi::host::MpoState st;
    mppi::host::mpo_reset(st, lambda0, epsilon, lr);
    const float lam0 = (float)lambda0, temp0 = st.temperature();
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(h->search.mpo_dev, &st, sizeof(st), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->search.mpo_temp_dev, &temp0, sizeof(float), hipMemcpyHostToDevice));
    if (!lambda_too) return MPPI_OK;  // (mppi_create: the dual exists, but no temperature has been asked for yet)
    HIP_TRY(h, hipMemcpy(h->search.lambda_dev, &lam0, sizeof(float), hipMemcpyHostToDevice));  // the first solve's temperature
    h->search.mirror.host->lam_next = h->search.mirror.host->lam_used = lambda0;
    h->search.lambda_dev_valid = true;
    return MPPI_OK;
}

}  // namespace mppi

extern "C" {

int mppi_softmax_stats(mppi_handle_t h, float lambda, double* out5_host, void* stream) {
    if (!h || !out5_host || !(lambda > 0.0f)) return fail(h, MPPI_E_INVALID, "bad softmax_stats arguments");
    hipStream_t s = (hipStream_t)stream;
    const unsigned* mk = h->min_key.cur();
    const int blocks = stats_blocks(h, BLOCK);
    hipLaunchKernelGGL(stats_partial_kernel, dim3(blocks), dim3(BLOCK), 0, s, h->core.costs, h->d.N, mk, lambda,
                       (const float*)nullptr, h->search.stats_part);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(stats_combine_kernel, dim3(1), dim3(WAVE), 0, s, h->search.stats_part, blocks, mk, &h->search.mirror.dev->single[0]);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));
    for (int i = 0; i < 5; ++i) out5_host[i] = h->search.mirror.host->single[i];
    return MPPI_OK;
}

int mppi_softmax_stats_multi(mppi_handle_t h, const float* lambdas_host, int count, double* out_host, void* stream) {
    if (!h || !lambdas_host || !out_host || count < 1 || count > STATS_L)
        return fail(h, MPPI_E_INVALID, "bad softmax_stats_multi arguments (1..32 lambdas)");
    float lam[STATS_L];
    for (int l = 0; l < STATS_L; ++l) {
        lam[l] = l < count ? lambdas_host[l] : 1.0f;
        if (!(lam[l] > 0.0f)) return fail(h, MPPI_E_INVALID, "lambda must be > 0");
    }
    hipStream_t s = (hipStream_t)stream;
    if (int rc = upload_small(h, h->search.lams_dev, lam, STATS_L, s)) return rc;
    const unsigned* mk = h->min_key.cur();
    const int blocks = stats_blocks(h);
    hipLaunchKernelGGL(stats_multi_kernel, dim3(blocks), dim3(STATS_THREADS), 0, s, h->core.costs, h->d.N, mk,
                       (const float*)h->search.lams_dev, h->search.stats_part, (float*)nullptr);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(stats_multi_combine_kernel, dim3(1), dim3(1024), 0, s, h->search.stats_part, blocks, &h->search.mirror.dev->grid[0]);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));
    for (int j = 0; j < count * 3; ++j) out_host[j] = h->search.mirror.host->grid[j];
    return MPPI_OK;
}

// ESSPS with no host synchronisation (mppi.py:351-370): statistics pass over the preset round-0 grid -> select
// (end-point rules / refined grid, on the device) -> statistics pass over that grid -> select (root) -> the
// temperature stays in HBM, where mppi_weights_reduce / mppi_finalize read it when called with MPPI_LAMBDA_DEVICE;
// mppi_get_lambda fetches it (synchronises).  Same arithmetic as mppi_essps_lambda: both run host_search.hpp.
int mppi_essps_lambda_device(mppi_handle_t h, double target_ess, double lam_min, double lam_max, void* stream) {
    if (int rc = check_essps(h, h != nullptr, target_ess, lam_min, lam_max)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = essps_prepare(h, lam_min, lam_max)) return rc;
    const unsigned* mk = h->min_key.cur();
    const int blocks = stats_blocks(h);
    double* host_lam = &h->search.mirror.dev->lam_next;
    float* lams0 = h->search.lams_dev + STATS_L;
    float* lams1 = h->search.lams_dev + 2 * STATS_L;
    for (int r = 0; r < 2; ++r) {
        const unsigned tag = next_tag(h->seq.round1);
        if (r == 0 && !h->opt.essps_merge0) {
            hipLaunchKernelGGL(stats_multi_kernel, dim3(blocks), dim3(STATS_THREADS), 0, s, h->core.costs, h->d.N, mk,
                               (const float*)lams0, h->search.stats_part, (float*)nullptr);
            hipLaunchKernelGGL(essps_select_kernel, dim3(1), dim3(1024), 0, s, (const float*)h->search.stats_part, blocks, target_ess,
                               h->search.essps_range, h->search.essps_dev, lams1, lams0, h->search.lambda_dev, host_lam);
        } else
            hipLaunchKernelGGL(r == 0 ? essps_round_kernel<0> : essps_round_kernel<1>, dim3(blocks), dim3(STATS_THREADS), 0, s, h->core.costs,
                               h->d.N, mk, target_ess, h->search.essps_range, h->search.essps_dev, lams1, lams0, h->search.lambda_dev, host_lam,
                               h->search.round1_cells, tag);
    }
    HIP_TRY(h, hipGetLastError());
    h->search.lambda_dev_valid = true;
    return MPPI_OK;
}

// The state the device-resident ESSPS search carries from one solve to the next, as an opaque blob for callers that save a
// solver and restore it elsewhere (mppi_clone_state copies the same buffers between two handles): {lam_min, lam_max} the first
// grid was built for, EsspsDev (the first grid of the NEXT search and its logs, left behind by the last one) and the three
// fp32 grids.  A search restored from it continues bit for bit.  Set-up path: both synchronise the device.
static constexpr size_t ESSPS_STATE_BYTES = 2 * sizeof(double) + sizeof(EsspsDev) + sizeof(float) * 3 * STATS_L;
int mppi_essps_get_state(mppi_handle_t h, void* out_host, int64_t* bytes_out_host) {
    if (!h || !bytes_out_host) return fail(h, MPPI_E_INVALID, "null");
    const bool any = h->search.essps_lo > 0.0;  // (no search has run on this handle yet: nothing to carry)
    *bytes_out_host = any ? (int64_t)ESSPS_STATE_BYTES : 0;
    if (!out_host || !any) return MPPI_OK;
    char* o = (char*)out_host;
    const double range[2] = {h->search.essps_lo, h->search.essps_hi};
    HIP_TRY(h, hipDeviceSynchronize());
    memcpy(o, range, sizeof(range));
    HIP_TRY(h, hipMemcpy(o + sizeof(range), h->search.essps_dev, sizeof(EsspsDev), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(o + sizeof(range) + sizeof(EsspsDev), h->search.lams_dev, sizeof(float) * 3 * STATS_L, hipMemcpyDeviceToHost));
    return MPPI_OK;
}

int mppi_essps_set_state(mppi_handle_t h, const void* in_host, int64_t bytes) {
    if (!h || !in_host) return fail(h, MPPI_E_INVALID, "null");
    if (bytes != (int64_t)ESSPS_STATE_BYTES) return fail(h, MPPI_E_INVALID, "essps state: a blob of another size (another build wrote it)");
    const char* in = (const char*)in_host;
    double range[2];
    memcpy(range, in, sizeof(range));
    if (int rc = check_essps(h, true, 1.0, range[0], range[1])) return rc;
    if (int rc = essps_prepare(h, range[0], range[1])) return rc;  // (the range and its logs; the cold grid is overwritten below)
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(h->search.essps_dev, in + sizeof(range), sizeof(EsspsDev), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->search.lams_dev, in + sizeof(range) + sizeof(EsspsDev), sizeof(float) * 3 * STATS_L, hipMemcpyHostToDevice));
    return MPPI_OK;
}

// The temperature a device-resident rule left behind (and, optionally, the one the last solve's weights used: the same
// for ESSPS / LBPS, the previous one for MPO).  Synchronises the stream.
int mppi_get_lambda(mppi_handle_t h, double* lambda_out_host, double* lambda_used_out_host, void* stream) {
    if (!h || !lambda_out_host) return fail(h, MPPI_E_INVALID, "null");
    if (!h->search.lambda_dev_valid) return fail(h, MPPI_E_STATE, "no temperature on the device");
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    *lambda_out_host = h->search.mirror.host->lam_next;
    if (lambda_used_out_host) *lambda_used_out_host = h->search.mirror.host->lam_used;
    return MPPI_OK;
}

// Passes over the costs (32-temperature grids) the last device-resident ESSPS / LBPS search took: ESSPS 1 when an
// end-point rule decided or the warm-started first grid was enough, else 2; LBPS always LBPS_ROUNDS.  Synchronises.
int mppi_search_passes(mppi_handle_t h, void* stream) {
    if (!h || !h->search.lambda_dev_valid) return 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return 0;
    return (int)h->search.mirror.host->passes;
}

// LBPS with no host synchronisation (mppi.py:341-349): LBPS_ROUNDS x (32-temperature statistics pass -> one-block
// grid step), the temperature stays in HBM (MPPI_LAMBDA_DEVICE).  See lbps_select_kernel.
int mppi_lbps_lambda_device(mppi_handle_t h, double delta, double lam_min, double lam_max, void* stream) {
    if (int rc = check_lbps(h, h != nullptr, delta, lam_min, lam_max)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float* lams0 = h->search.lams_dev;              // (the caller's-grid slot doubles as LBPS's preset round-0 grid)
    float* lams1 = h->search.lams_dev + 2 * STATS_L;
    LbpsDev st{};
    float lamf[STATS_L];
    mppi::host::essps_make_grid<STATS_L>(lam_min, lam_max, st.grid0);
    for (int j = 0; j < STATS_L; ++j) { lamf[j] = (float)st.grid0[j]; st.grid[j] = st.grid0[j]; }
    if (h->search.lbps_lo != lam_min || h->search.lbps_hi != lam_max) {  // another range: the search state too (set-up path, blocking)
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, hipMemcpy(h->search.lbps_dev, &st, sizeof(st), hipMemcpyHostToDevice));
        h->search.lbps_lo = lam_min; h->search.lbps_hi = lam_max;
    }
    // the caller's-grid slot may have been overwritten by mppi_softmax_stats_multi: refresh it
    if (int rc = upload_small(h, lams0, lamf, STATS_L, s)) return rc;
    const unsigned* mk = h->min_key.cur();
    const int blocks = stats_blocks(h);
    for (int r = 0; r < LBPS_ROUNDS; ++r) {
        hipLaunchKernelGGL(stats_multi_kernel, dim3(blocks), dim3(STATS_THREADS), 0, s, h->core.costs, h->d.N, mk,
                           (const float*)(r == 0 ? lams0 : lams1), h->search.stats_part, h->search.stats_max);
        auto select = lbps_select_kernel<false, true>;  // <LAST, FIRST>: the rounds differ in nothing else
        if (r > 0) select = r < LBPS_ROUNDS - 1 ? lbps_select_kernel<false, false> : lbps_select_kernel<true, false>;
        hipLaunchKernelGGL(select, dim3(1), dim3(1024), 0, s, (const float*)h->search.stats_part, (const float*)h->search.stats_max, blocks,
                           mk, delta, h->search.lbps_dev, lams1, h->search.lambda_dev, &h->search.mirror.dev->lam_next);
    }
    HIP_TRY(h, hipGetLastError());
    h->search.lambda_dev_valid = true;
    return MPPI_OK;
}

// ESSPS temperature (mppi.py:351-370,559-566): the root of ESS(lambda) = target on [lam_min, lam_max] with the
// reference's end-point rules, found on the host from device statistics — two 32-point geometric grids
// (mppi_softmax_stats_multi: one pass over the costs each) and an inverse polynomial interpolation in
// (ESS, log lambda): host::essps_lambda in host_search.hpp.  Same algorithm as pi_mpc/_host.py::essps_lambda_grid
// (which sharded solvers use, with an all_gather per grid); kept in the library so that the single-GPU solve has no
// interpreter work per probe.
int mppi_essps_lambda(mppi_handle_t h, double target_ess, double lam_min, double lam_max, double* lambda_out,
                      void* stream) {
    if (int rc = check_essps(h, h && lambda_out, target_ess, lam_min, lam_max)) return rc;
    constexpr int P = STATS_L;
    int rc = MPPI_OK;
    if (h->search.essps_prev_lo != lam_min || h->search.essps_prev_hi != lam_max) h->search.essps_prev_host.warm = false;  // another range: a cold search
    const bool ok = mppi::host::essps_lambda<P>(
        [&](const double* grid, double* ess) {
            float lamf[P];
            double raw[P * 3];
            for (int j = 0; j < P; ++j) lamf[j] = (float)grid[j];
            rc = mppi_softmax_stats_multi(h, lamf, P, raw, stream);
            if (rc) return false;
            for (int j = 0; j < P; ++j) ess[j] = raw[3 * j] * raw[3 * j] / raw[3 * j + 1];
            return true;
        },
        target_ess, lam_min, lam_max, *lambda_out, h->search.essps_prev_host);
    h->search.essps_prev_lo = lam_min; h->search.essps_prev_hi = lam_max;
    if (!ok) h->search.essps_prev_host.warm = false;
    return ok ? MPPI_OK : rc;
}

// LBPS as the reference searches it (mppi.py:341-349: scipy's bounded Brent, host::fminbound step for step) with NO host
// synchronisation: ONE launch of lbps_brent_kernel (mppi_search.hpp) runs every probe — the statistics of
// mppi_softmax_stats bit for bit, gathered by every block through tagged cells — and leaves the temperature in HBM
// (MPPI_LAMBDA_DEVICE) and in mapped host memory.  The same temperature as mppi_lbps_lambda, to the bit.
int mppi_lbps_brent_device(mppi_handle_t h, double delta, double lam_min, double lam_max, void* stream) {
    if (int rc = check_lbps(h, h != nullptr, delta, lam_min, lam_max)) return rc;
    hipStream_t s = (hipStream_t)stream;
    // the geometry of mppi_softmax_stats (stats_partial_kernel): nvb blocks of 256 threads, grid-stride over the costs;
    // block l of this launch runs the virtual blocks l, l + 64, ... (lane l's rows of stats_combine_kernel)
    const int nvb = stats_blocks(h, BLOCK);
    const int64_t per_thread64 = (h->d.N + (int64_t)nvb * BLOCK - 1) / ((int64_t)nvb * BLOCK);
    const int grid = std::min(nvb, BRENT_LANES);
    const int threads = BLOCK * ((nvb + BRENT_LANES - 1) / BRENT_LANES);
    if (grid > h->cu_count) return fail(h, MPPI_E_STATE, "lbps_brent: more blocks than CUs (they must be resident at once)");
    int per_thread = (int)std::min<int64_t>(per_thread64, BRENT_STAGE_MAX + 1);  // (beyond the staging limit only the flag matters)
    size_t shmem = per_thread <= BRENT_STAGE_MAX ? sizeof(float) * BrentStageLds::floats(per_thread, threads) : 0;
    if (shmem + sizeof(BrentLds) + 256 > (size_t)h->lds_max) { per_thread = BRENT_STAGE_MAX + 1; shmem = 0; }
    if (shmem > 48 * 1024) {
        static size_t granted = 0;  // (per process: the attribute belongs to the kernel, not to a handle)
        if (shmem > granted) {
            (void)hipFuncSetAttribute((const void*)lbps_brent_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
            (void)hipGetLastError();
            granted = shmem;
        }
    }
    if (h->seq.brent > 0xFFFFFFFFu - 2 * BRENT_SEQ_STRIDE) {  // tag space used up (after 8 million searches): start over on clean cells
        HIP_TRY(h, hipMemsetAsync(h->search.brent_cells, 0, sizeof(unsigned long long) * 2 * BRENT_LANES * BRENT_CELLS, s));
        h->seq.brent = 0;
    }
    const BrentCtx bx{h->search.brent_cells, h->search.error.dev, h->seq.brent, h->opt.fused_timeout_ticks};
    h->seq.brent += BRENT_SEQ_STRIDE;
    // (test hook: with the last block missing, its lane's sums never arrive — what a block that is not resident looks like to
    // the others: every poll runs into the budget, the flag is raised and the temperature is NaN)
    hipLaunchKernelGGL(lbps_brent_kernel, dim3(grid - (h->search.brent_drop_block && grid > 1 ? 1 : 0)), dim3(threads), shmem, s, (const float*)h->core.costs, h->d.N,
                       h->min_key.cur(), nvb, per_thread, delta, lam_min, lam_max, bx, h->search.lambda_dev,
                       &h->search.mirror.dev->lam_next);
    HIP_TRY(h, hipGetLastError());
    h->search.lambda_dev_valid = true;
    return MPPI_OK;
}

// 1 once a poll of a device-resident temperature search timed out on this handle (a block of lbps_brent_kernel never became
// resident: the GPU is shared with other work): that solve's temperature — and with it its outputs — are NaN.
int mppi_search_error(mppi_handle_t h) { return h ? h->search.error.get() : 0; }

#ifdef MPPI_BRENT_TRACE
extern "C" int mppi_debug_brent_trace(mppi_handle_t h, int* out8) {  // 10 ns ticks of the last search per phase (block 0)
    if (!h || !h->search.error.host) return MPPI_E_STATE;
    (void)hipDeviceSynchronize();
    for (int k = 0; k < 8; ++k) out8[k] = h->search.error.host[1 + k];
    return MPPI_OK;
}
#endif

// LBPS temperature (mppi.py:341-349,534-557): scipy's bounded Brent minimiser (host::fminbound, xatol 1e-5) of the
// lower-bound objective over [lam_min, lam_max]; every probe is one mppi_softmax_stats round trip (two tiny launches
// + a 40-byte read-back through mapped host memory), with no interpreter in the loop.  Unsharded handles; synchronises.
int mppi_lbps_lambda(mppi_handle_t h, double delta, double lam_min, double lam_max, double* lambda_out, void* stream) {
    if (int rc = check_lbps(h, h && lambda_out, delta, lam_min, lam_max)) return rc;
    int rc = MPPI_OK;
    const bool ok = mppi::host::lbps_lambda(
        [&](double lam, mppi::host::SoftmaxStats& st) {
            double o[5];
            rc = mppi_softmax_stats(h, (float)lam, o, stream);
            if (rc) return false;
            st = mppi::host::SoftmaxStats{o[0], o[1], o[2], o[3], o[4]};
            return true;
        },
        delta, lam_min, lam_max, *lambda_out);
    return ok ? MPPI_OK : rc;
}

// MPO temperature (mppi.py:191-200,387-398): the dual variable log T and its Adam moments live in DEVICE memory.
int mppi_mpo_reset(mppi_handle_t h, double lambda0, double epsilon, double lr) {
    if (!h || !(lambda0 > 0.0) || !(lr > 0.0)) return fail(h, MPPI_E_INVALID, "bad mpo arguments");
    return mpo_upload(h, lambda0, epsilon, lr, true);
}

// One Adam step of the dual on the last solve's costs with NO host synchronisation: statistics at softplus(logT) (read
// from device memory) + a one-thread step; lambda = exp(logT) — the temperature of the NEXT solve — replaces the one in
// HBM that this solve's weights used (MPPI_LAMBDA_DEVICE).  Call it after mppi_finalize.
int mppi_mpo_step_device(mppi_handle_t h, void* stream) {
    if (!h) return MPPI_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const unsigned* mk = h->min_key.cur();
    const int blocks = stats_blocks(h, BLOCK);
    hipLaunchKernelGGL(stats_partial_kernel, dim3(blocks), dim3(BLOCK), 0, s, h->core.costs, h->d.N, mk, 1.0f,
                       (const float*)h->search.mpo_temp_dev, h->search.stats_part);
    hipLaunchKernelGGL(mpo_step_kernel, dim3(1), dim3(WAVE), 0, s, (const float*)h->search.stats_part, blocks, mk, h->search.mpo_dev,
                       h->search.lambda_dev, h->search.mpo_temp_dev, &h->search.mirror.dev->lam_next);
    HIP_TRY(h, hipGetLastError());
    h->search.lambda_dev_valid = true;
    return MPPI_OK;
}

// The same step, returning lambda_out = exp(logT) = the temperature of the NEXT solve.  Unsharded handles; synchronises.
int mppi_mpo_step(mppi_handle_t h, double* lambda_out, void* stream) {
    if (!h || !lambda_out) return fail(h, MPPI_E_INVALID, "null");
    if (int rc = mppi_mpo_step_device(h, stream)) return rc;
    return mppi_get_lambda(h, lambda_out, nullptr, stream);
}

// {log T, first moment, second moment, step count} of the dual (inspection / tests).  Synchronises the device.
int mppi_mpo_state(mppi_handle_t h, double* out4_host) {
    if (!h || !out4_host) return fail(h, MPPI_E_INVALID, "null");
    mppi::host::MpoState st;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(&st, h->search.mpo_dev, sizeof(st), hipMemcpyDeviceToHost));
    out4_host[0] = st.log_temperature; out4_host[1] = st.m; out4_host[2] = st.v; out4_host[3] = st.t;
    return MPPI_OK;
}

// The inverse of mppi_mpo_state (restoring a saved solver): {log T, first moment, second moment, step count} -> the dual; the
// temperature of the next solve becomes exp(log T) (mppi.py:398).  epsilon / lr keep their values.  Synchronises the device.
int mppi_mpo_set_state(mppi_handle_t h, const double* in4_host) {
    if (!h || !in4_host) return fail(h, MPPI_E_INVALID, "null");
    mppi::host::MpoState st;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(&st, h->search.mpo_dev, sizeof(st), hipMemcpyDeviceToHost));
    st.log_temperature = (float)in4_host[0]; st.m = (float)in4_host[1]; st.v = (float)in4_host[2]; st.t = (int32_t)in4_host[3];
    const float temp = st.temperature(), lam = (float)exp(st.log_temperature);
    HIP_TRY(h, hipMemcpy(h->search.mpo_dev, &st, sizeof(st), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->search.mpo_temp_dev, &temp, sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->search.lambda_dev, &lam, sizeof(float), hipMemcpyHostToDevice));
    h->search.mirror.host->lam_next = h->search.mirror.host->lam_used = (double)lam;
    h->search.lambda_dev_valid = true;
    return MPPI_OK;
}

// Device address of the dual's log T (one fp32, first field of the state mppi_mpo_step_device updates): lets a caller
// expose it without a copy (this build's MPPI makes it the storage of its `log_temperature` nn.Parameter, mppi.py:194-199).
// Read-only for the caller: the library derives the temperatures it uses when the dual steps.
int mppi_mpo_log_temperature_ptr(mppi_handle_t h, float** out_dev) {
    if (!h || !out_dev || !h->search.mpo_dev) return fail(h, MPPI_E_INVALID, "null");
    *out_dev = &h->search.mpo_dev.p->log_temperature;
    return MPPI_OK;
}

}  // extern "C"
