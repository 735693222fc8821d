// mppi_rollout_kernel.inc — the text of the rollout kernel, included twice by mppi_rollout.hpp: as rollout_cost_kernel
// (MPPI_ROLLOUT_AC 0) and, with the opt-in control-cost term (mppi_action_cost.hpp), as rollout_action_cost_kernel
// (MPPI_ROLLOUT_AC 1: one more launch argument, 4R more floats of LDS for g).  One text, so that the kernel without the
// term is compiled from exactly what it was compiled from before the term existed: same name, arguments and registers.
template <int MODEL, int FAST, bool GEN, bool UC, bool TRACK = false>
__global__ __launch_bounds__(BLOCK) MPPI_ROLLOUT_ATTR void MPPI_ROLLOUT_KERNEL(const float4* __restrict__ noise,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ x0,
                                                             float* __restrict__ costs,
                                                             unsigned* __restrict__ min_key,
                                                             unsigned* __restrict__ next_min_key,
                                                             float* __restrict__ mean_used,
                                                             float* __restrict__ x0_used, Dims d, GenCtx gen,
                                                             ModelCtx ctx, const float* __restrict__ b1_in,
                                                             float* __restrict__ b1_state_out,
                                                             unsigned long long* __restrict__ stamps
#if MPPI_ROLLOUT_AC
                                                             , ActionCostArgs ac
#endif
                                                             ) {
    using M = ModelT<MODEL, FAST>;
    __shared__ float s_min[BLOCK / WAVE];
    // `stamps` (or null: untimed) is the launch's pair of 100 MHz wall-clock stamps {start, end} (StageTimer): block 0, which
    // is dispatched first, stores the start; every block raises the end as its last act.  end - start runs from block 0's
    // first instruction to the last block's last one: the stage's time as seen from inside the dispatch.
    // The pointer waits for the end of the block in LDS, not in a pair of SGPRs held across the horizon loop: six more live
    // SGPRs took the kernel from eight waves per SIMD to seven.  `costs` and `min_key` wait there too: the loop's second
    // bound (trajectory_cost, "Even drain") needs the registers (racing: 103 SGPRs and seven waves per SIMD without, 99 with).
    ROLLOUT_TRACE(0);
    ROLLOUT_TRACE(5);
    __shared__ unsigned long long* s_stamps;
    __shared__ float* s_costs;
    __shared__ unsigned* s_min_key;
#if MPPI_ROLLOUT_AC
    // kappa = weight * lambda: the temperature is read through its pointer here, once per block, and waits in LDS too
    __shared__ float s_kappa;
    if (threadIdx.x == 0) s_kappa = action_cost_kappa(ac.weight, ac.lambda_dev ? *ac.lambda_dev : ac.lambda);
#endif
    if (threadIdx.x == 0) {
        s_stamps = stamps;
        s_costs = costs;
        s_min_key = min_key;
        if (stamps != nullptr && blockIdx.x == 0) stamps[0] = wall_clock64();
    }
    // (The learned models' instantiations with the tracking cost: the pointer and the weight of the terminal value wait for the
    // end of the horizon loop in LDS as well — three more scalar registers held across it took mlp84's library-math tile kernel
    // from 80 to 81 VGPRs and six waves per SIMD to five, and mlp41's library-math control-cost kernel from 96 to 97 and five
    // to four.  Every other instantiation: no slot, no code.)
    const MlpValueSlot* vslot = nullptr;
    if constexpr (is_mlp(MODEL) && TRACK) {
        __shared__ MlpValueSlot s_value;
        if (threadIdx.x == 0) {
            s_value.table = reinterpret_cast<const float*>(ctx.maps[1].cells);
            s_value.weight = ctx.maps[1].cell;
            s_value.n = d.N;
        }
        vslot = &s_value;
    }
    // RolloutLds: [4*R] mean groups, [4*R] zeros (samples that do not inherit the mean), (with the control-cost term: [4*R] g =
    // mean * inv_covariance,) then [T*KROW] step rows
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    // One extra block (the last) when the PREVIOUS solve left its state sequence pending (option "lazy_state_seq"): the
    // batch-1 rollout of that solution (mppi.py:448-449) from the inputs finalize_kernel left in b1_in — T dependent steps
    // of one wave, hidden behind this launch's N-sample rollout instead of extending the previous solve's tail.
    if (b1_state_out != nullptr && blockIdx.x == gridDim.x - 1) {
        for (int i = threadIdx.x; i < d.row + M::DS; i += BLOCK) s_dyn[i] = b1_in[i];
        __syncthreads();
        batch1_rollout<MODEL, FAST>(ctx, s_dyn + RolloutLds::rider_x0(d.row), s_dyn, d.T, b1_state_out);
        if (stamps != nullptr && threadIdx.x == 0) (void)atomicMax(stamps + 1, (unsigned long long)wall_clock64());
        return;
    }
#ifdef MPPI_AB_VGPR_FLOOR  // (A/B knob of scripts/build_variant.sh: same code at the occupancy of an 85-VGPR build)
    asm volatile("; vgpr floor" ::: "v84");
#endif
    // the state this solve starts from outlives the caller's buffer (mppi_bind_state is zero-copy): later
    // re-rolls of this solve's samples (get_top_samples, _state_seq_batch) read the snapshot
    if (blockIdx.x == 0 && threadIdx.x < M::DS) x0_used[threadIdx.x] = x0[threadIdx.x];
    float4* s_mean4 = reinterpret_cast<float4*>(s_dyn);
    float* s_ktab = s_dyn + RolloutLds::ktab(d.R, MPPI_ROLLOUT_AC != 0);
    for (int f = threadIdx.x; f < 4 * d.R; f += BLOCK) {
        const float m = f < d.row ? mean[f] : 0.0f;
        s_dyn[f] = m;
        s_dyn[RolloutLds::zeros(d.R) + f] = 0.0f;
#if MPPI_ROLLOUT_AC
        {   // row 0 of the inverse covariance is zero (action_cost_inv); zeros past the row
            float g = 0.0f;
            if (f >= M::DC && f < d.row) {
                const float sg = ac.sigtab ? ac.sigtab[f] : d.sigma[f % M::DC];
                g = action_cost_g(m, action_cost_inv(f / M::DC, sg));
            }
            s_dyn[RolloutLds::g(d.R) + f] = g;
        }
#endif
        // the mean this solve samples around outlives the warm-start update (get_top_samples re-rolls with it)
        if (blockIdx.x == 0 && f < d.row) mean_used[f] = m;
    }
    for (int f = threadIdx.x; f < d.T * M::KROW; f += BLOCK) s_ktab[f] = ctx.ref[f];
    __syncthreads();
    ROLLOUT_TRACE(1);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * (BLOCK / WAVE) + wid;
    // the minimum key is double-buffered: this launch accumulates into `min_key` (reset by the
    // previous launch) and resets the other slot for the next one -> no memset between solves
    if (blockIdx.x == 0 && threadIdx.x == 0) *next_min_key = 0xFFFFFFFFu;
    float total = INFINITY;
    if (tile < d.tiles) {
        const int64_t i = tile * 64 + lane;
        const uint64_t gi = (uint64_t)(d.sample_offset + i);
        const bool inherit = (d.sample_offset + i) < d.inherit_count;
        const float4* np = noise + tile * d.R * 64 + lane;
        bool bad = false;
        const float4* mp = inherit ? s_mean4 : s_mean4 + d.R;  // (RolloutLds::zeros, in float4 groups)
#if MPPI_ROLLOUT_AC
        total = lane_cost<MODEL, FAST, GEN, UC, true, TRACK, is_mlp(MODEL) && TRACK>(np, gi, gen, mp, s_ktab, x0, d, ctx, s_mean4 + 2 * d.R /* RolloutLds::g, in float4 groups */, &s_kappa, vslot);
#else
        total = lane_cost<MODEL, FAST, GEN, UC, false, TRACK, is_mlp(MODEL) && TRACK>(np, gi, gen, mp, s_ktab, x0, d, ctx, nullptr, nullptr, vslot);
#endif
        int64_t n = d.N;  // (with the slot: read back from it — the sample count is then no scalar pair held across the loop)
        if constexpr (is_mlp(MODEL) && TRACK) n = static_cast<const volatile MlpValueSlot*>(vslot)->n;
        if (i < n) s_costs[i] = total;
        else total = INFINITY;
    }
    const float wm = wave_min(total);
    if (lane == 0) s_min[wid] = wm;
    __syncthreads();
    ROLLOUT_TRACE(4);
    // (The learned models' instantiations with the tracking cost form this test anew: the compiler otherwise keeps the lane mask of the `threadIdx.x == 0` at the top of
    // the kernel in a scalar register pair across the horizon loop (here: from the mask of `lane == 0`, which is held anyway, and the
    // wave's index as a scalar), and their loop has none to spare — mlp84's library-math tile
    // kernel spilled the pair into a vector lane, 80 -> 81 VGPRs and six waves per SIMD -> five, and mlp41's library-math
    // control-cost kernel 96 -> 97 and five -> four.  Every other model: the text it was.)
    bool first_thread = threadIdx.x == 0;
    if constexpr (is_mlp(MODEL) && TRACK) first_thread = lane == 0 && __builtin_amdgcn_readfirstlane(wid) == 0;
    if (first_thread) {
        float m = s_min[0];
#pragma unroll
        for (int w = 1; w < BLOCK / WAVE; ++w) m = fminf(m, s_min[w]);
        if (m < INFINITY) atomicMin(s_min_key, float_to_key(m));
        unsigned long long* const st = s_stamps;
        if (st != nullptr) (void)atomicMax(st + 1, (unsigned long long)wall_clock64());
    }
}

