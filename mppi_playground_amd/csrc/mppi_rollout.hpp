// mppi_rollout.hpp — Steps 1b-3 (mppi.py:266-336): clamp, N x T rollout and stage / terminal costs — rollout_cost_kernel (lane per trajectory) and the literal wavefront-per-trajectory variant.
// Part of the MPPI.forward() hot path for gfx950; see mppi_handle.hpp for the map of the files.
#pragma once
#include "mppi_action_cost.hpp"
#include "mppi_lds.hpp"
#include "mppi_sample.hpp"

namespace mppi {

// -DMPPI_ROLLOUT_TRACE (experiments only: scripts/rollout_timeline.py): lane 0 of every wave of rollout_cost_kernel stores the
// 100 MHz clock at its entry (0), behind the prologue's barrier (1), at the entry and the exit of the horizon loop (2) and
// at the end of its block (4), and where it ran (5: HW_REG_HW_ID, HW_REG_XCC_ID << 32), into row `tile` of a [tiles][6] buffer
// that mppi_debug_rollout_trace() hands in.  The loop's two stamps are one store behind the loop, the low words of the clock
// in column 2 (entry | exit << 32; column 3 stays 0): the entry's word waits in ONE scalar register (a store in front of the
// loop, or a register pair across it, costs the racing kernel a wave per SIMD).
// Off in the product: no code, no symbol.
#ifdef MPPI_ROLLOUT_TRACE
static __device__ unsigned long long* g_rollout_trace;
__device__ __forceinline__ void rollout_trace(int k) {
    unsigned long long* const rows = *(unsigned long long* volatile*)&g_rollout_trace;  // (read again at every stamp: not held across the loop)
    if (rows == nullptr || (threadIdx.x & 63) != 0) return;
    unsigned long long v = (unsigned long long)wall_clock64();
    if (k == 5)  // s_getreg_b32 hwreg(id, 0, 32): id | (32 - 1) << 11; HW_ID = 4, XCC_ID = 20
        v = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
            (unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32;
    rows[((size_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6)) * 6 + k] = v;
}
__device__ __forceinline__ void rollout_trace_loop(unsigned entry_lo) {
    unsigned long long* const rows = *(unsigned long long* volatile*)&g_rollout_trace;
    if (rows == nullptr) return;  // (every lane stores the same word to a wave-uniform address: no divergent branch, two data VGPRs)
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    rows[((size_t)blockIdx.x * (BLOCK / WAVE) + wid) * 6 + 2] = (unsigned long long)(unsigned)wall_clock64() << 32 | entry_lo;
}
#define ROLLOUT_TRACE(k) rollout_trace(k)
#define ROLLOUT_TRACE_LOOP_ENTRY() const unsigned trace_entry_lo = (unsigned)wall_clock64()
#define ROLLOUT_TRACE_LOOP_EXIT() rollout_trace_loop(trace_entry_lo)
#else
#define ROLLOUT_TRACE(k) do { } while (0)
#define ROLLOUT_TRACE_LOOP_ENTRY() do { } while (0)
#define ROLLOUT_TRACE_LOOP_EXIT() do { } while (0)
#endif

#ifdef MPPI_AB_NO_DRAIN_PRIO  // (A/B knob of scripts/build_variant.sh: the same code, every wave at priority 0 throughout)
#define MPPI_DRAIN_PRIO(p) __builtin_amdgcn_s_setprio(0)
#else
#define MPPI_DRAIN_PRIO(p) __builtin_amdgcn_s_setprio(p)
#endif

// ------------------------------------------------------------------------------------------
// Steps 1b-3 fused: U = clamp(mean + eps), rollout, stage + terminal cost (mppi.py:266-336).
// Reads the noise once (16 B per lane per 4/dc steps), writes costs[N] and the shard minimum.
//
// trajectory_cost(): one lane walks one trajectory.  `np` points at the lane's first float4 of the
// tile; consecutive groups are 64 float4 apart.
// `mean4` (R float4 groups, same grouping as the noise row; lanes beyond the exploration threshold
// are handed an all-zero copy, mppi.py:266-270) and `ktab` (KROW floats per step) are the
// block's LDS copies of the wave-uniform per-step inputs: LDS returns in order, so the compiler can
// keep the fetch of the next group / next row in flight (lgkmcnt(N)) while the current step computes,
// which scalar (SMEM) loads — out of order, lgkmcnt(0) only — do not allow.
// UC: the solver's clamp range lies inside the model's own action clamp (compile-time so that the
// second clamp disappears).
// VAR: a launch-uniform model variant the kernel has branched on OUTSIDE the horizon loop (racing: unit wheel base).
// X0OUT (models with EntryGeneral only): the start lies outside the model's position clamp — launch-uniform, x0 is the
// same for every lane — so the stage cost of step 0 takes the bounds-tested map lookup (every later state is clamped).
// AC: the opt-in control-cost term (mppi.py:294-316,330-336; mppi_action_cost.hpp).  `g4` is the block's LDS copy of
// g = mean * inv_covariance in the grouping of `mean4` — the REAL mean for every lane, exploration lanes included
// (mppi.py:313) — read one group at a time where its steps run (no look-ahead: four VGPRs instead of eight); the lane
// accumulates A = sum g * U over its solver-clamped actions and adds kappa * A behind the cost sum.  `kappa` waits in LDS
// (see rollout_cost_kernel on what SGPRs held across the loop cost).  Off: no code, `g4` and `kappa` are null.
// TRACK (the learned models only; every kernel that walks them carries it as its last template argument): the instantiation
// with the tracking cost (reference table, angular mask: MlpModel::cost).  TRACK = false is the kernel of a handle with
// neither, compiled from the text it was compiled from before the tracking cost existed (MlpModel::cost_plain; same
// registers, same code): the launch sites pick one per launch (mlp_tracking), so the choice is made outside the horizon loop
// and a default solver runs the kernel it ran.
template <int MODEL, int FAST, bool GEN, bool UC, bool VAR = false, bool X0OUT = false, bool AC = false, bool TRACK = false,
          bool SLOT = false>
__device__ __forceinline__ float trajectory_cost(const float4* __restrict__ np, uint64_t gi, const GenCtx& gen,
                                                 const float4* mean4, const float* ktab,
                                                 const float* __restrict__ x0, const Dims& d, const ModelCtx& ctx_in,
                                                 bool& bad, const float4* g4 = nullptr, const float* kappa = nullptr,
                                                 const MlpValueSlot* vslot = nullptr) {
    using M = ModelT<MODEL, FAST>;
    using K = typename M::K;
    constexpr int DS = M::DS, DC = M::DC, SPG = 4 / DC;
    // wave-uniform operands that would otherwise cost a v_mov per use inside the loop (a VALU instruction reads one scalar
    // register): the model's picks of its launch constants (Model::pin_hot) and the Philox key of round 0
    ModelCtx ctx = ctx_in;
    if constexpr (FAST != 0 && EntryGeneral<M>::value) M::pin_hot(ctx);
    KeyPins pins{gen.seed_lo, gen.seed_hi, gen.seed_lo + 0x9E3779B9u};
    // The three-instruction u1 of box_muller (philox.hpp) keeps 2^-24 in a vector register.  The rollout kernels of the goal
    // zone sit at 80 VGPRs, the last count with six waves per SIMD, and the learned model's control-cost kernel at 96, the
    // last with five: with it they lose a wave (82 / 97), so these models draw with the four-instruction form, the same bits.
    // The 8-state learned models take it: it costs each of their regenerating kernels one VGPR (mlp81 94 -> 95, mlp82 97 -> 98,
    // mlp84 93 -> 94 at the fast level; 99 -> 100, 102 -> 103, 81 -> 82 with the library math; the control-cost kernels alike)
    // and none of them crosses a step: the waves per SIMD are the same with either form (profiles/r25_mlp8.md).
    constexpr bool U1_FMA = MODEL != MPPI_MODEL_GOALZONE && MODEL != MPPI_MODEL_MLP41;
    if (GEN) asm volatile("" : "+v"(pins.k0v), "+v"(pins.k1v), "+v"(pins.k0w));
    float s[DS], pu[DC], pl[DC];
#pragma unroll
    for (int j = 0; j < DS; ++j) s[j] = x0[j];
    if (FAST) {
        if constexpr (EntryGeneral<M>::value) {
            M::enter_any(s);  // any finite heading, wrapped once by the reference's own operation (exact)
        } else {
            M::check_state(ctx, s, bad);
            M::enter(s);  // kinematic models: wrap the heading once; every later heading is a fixed point of that wrap
        }
    }
    // clamp bounds live in VGPRs: v_med3_f32 takes one SGPR operand only, and the compiler would
    // otherwise re-materialise the second bound with a v_mov in every step
    float lo[DC], hi[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        lo[k] = d.u_min[k]; hi[k] = d.u_max[k];
        asm volatile("" : "+v"(hi[k]));
    }
    CostSum<exact_cost_sum(MODEL)> acc;  // sum of the stage costs (mppi.py:333): exactly rounded (racing: sequential fp32)
    K knext = M::load_k(ktab, 0);
    float4 e = noise_group<GEN, U1_FMA>(np, 0, gi, gen, d, &pins);
    float4 m4 = mean4[0];
    {   // info["prev_action"] of step 0 is U[:, 0] itself (mppi.py:299-301)
        const float e0[4] = {e.x, e.y, e.z, e.w}, m0[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
        for (int k = 0; k < DC; ++k) pu[k] = pl[k] = clampf(m0[k] + e0[k], lo[k], hi[k]);
    }
    int t = 0;
    float A = 0.0f;  // (AC) sum over (t, k) of g * U, sequential fp32
    auto one_step = [&](const float* ev, const float* mv, const float* gv) {
        // (with the tracking cost the learned models' step constant is the step index itself: no look-ahead to keep in a register)
        K kcur = knext;
        if constexpr (is_mlp(MODEL) && TRACK) kcur = M::load_k(ktab, t);
        else knext = M::load_k(ktab, min(t + 1, d.T - 1));
        float u[DC];
#pragma unroll
        for (int k = 0; k < DC; ++k) u[k] = clampf(mv[k] + ev[k], lo[k], hi[k]);
        if constexpr (AC) {
#pragma unroll
            for (int k = 0; k < DC; ++k) A = action_cost_accumulate(A, gv[k], u[k]);
        }
        float sn[DS], ss[DS];
        if constexpr (is_racing_model(MODEL)) M::step(ctx, s, u, sn, ss, bad, UC, FAST != 0, VAR);
        else M::step(ctx, s, u, sn, ss, bad, UC, FAST != 0);
        if constexpr (is_mlp(MODEL) && !TRACK) acc.add(M::cost_plain(ctx, kcur, ss, u, pu, bad));
        else if constexpr (X0OUT) acc.add(M::cost(ctx, kcur, ss, u, pu, bad, t == 0));
        else acc.add(M::cost(ctx, kcur, ss, u, pu, bad));
#pragma unroll
        for (int k = 0; k < DC; ++k) { pl[k] = pu[k]; pu[k] = u[k]; }
#pragma unroll
        for (int j = 0; j < DS; ++j) s[j] = sn[j];
        ++t;
    };
    // The learned-dynamics models' step is some 4 KB of code (a layer of 32 units and its activations, unrolled: mppi_models.inc),
    // and every unrolled step of a float4 group below is a copy of it: 4 / DC steps x {two drain halves, epilogue} would be twelve
    // copies, most of the instruction cache.  Their groups are walked by a ROLLED loop instead: the step's inputs are picked
    // from the group's registers with selects on the (wave-uniform) step index — three per value, against ~1300 multiply-adds
    // per step — and each of the three walks holds one copy.  Same operations per step in the same order.
    constexpr bool ROLL_GROUP = is_mlp(MODEL);
    auto pick4 = [](float a0, float a1, float a2, float a3, int i) {  // (scalars: nothing here can be turned into an indexed load)
        float r = a0;
        r = i == 1 ? a1 : r;
        r = i == 2 ? a2 : r;
        r = i == 3 ? a3 : r;
        return r;
    };
    auto rolled_group = [&](const float4 ev, const float4 mv, const float4 gv, bool ragged) {
#pragma clang loop unroll(disable)
        for (int g = 0; g < SPG; ++g) {
            if (ragged && !(t < d.T)) break;
            float e1[DC], m1[DC], g1[DC];
#pragma unroll
            for (int k = 0; k < DC; ++k) {
                e1[k] = pick4(ev.x, ev.y, ev.z, ev.w, g * DC + k);
                m1[k] = pick4(mv.x, mv.y, mv.z, mv.w, g * DC + k);
                g1[k] = AC ? pick4(gv.x, gv.y, gv.z, gv.w, g * DC + k) : 0.0f;
            }
            one_step(e1, m1, g1);
        }
    };
    // Groups walked by the loops below: SPG steps each, no per-step bound checks.  Tiles: every group that lies completely
    // inside the horizon, d.T / SPG.  Regenerating loop: only the groups that still have a SUCCESSOR to generate,
    // (d.T - 1) / SPG.  An iteration of that loop generates the noise of the next group, a whole Philox4x32-10 and two
    // Box-Muller pairs; when T*dc is a multiple of 4 the last complete group is also the last group (d.T / SPG == d.R), the
    // clamped look-ahead would generate it a second time and nothing would read the result.  That group's steps go through
    // the ragged epilogue below instead, which consumes `e` and `m4` and generates nothing: the same operations per step
    // in the same order, the same order of the cost sum, R generations for R groups.  When T*dc is no multiple of 4 the
    // two bounds are equal.
    // Per model: the fast-math functors are compiled with FP contraction `fast` (mppi_models.hpp), and which product of a
    // sum becomes the FMA is the compiler's choice per copy of the step.  The move keeps every bit only where the loop's
    // and the epilogue's copies are contracted alike: held bit for bit against the tile loop for racing, nav2d and the
    // pendulum (tests/test_gpu_rollout_last_group.py).  The cart-pole's are not (stage cost a*a + 0.1*w*w + 0.1*x*x: a*a
    // is the bare product in the loop, 0.1*w*w in the epilogue; 6 % of the costs changed at T = 4 and 8), so it and the models
    // nobody has compared keep the loop over every complete group.
    constexpr bool LAST_GROUP_IN_EPILOGUE =
        GEN && (MODEL == MPPI_MODEL_RACING || MODEL == MPPI_MODEL_NAV2D || MODEL == MPPI_MODEL_PENDULUM);
    const int full = LAST_GROUP_IN_EPILOGUE ? (d.T - 1) / SPG : d.T / SPG;
    if (GEN) {
        // Even drain: VALU issue goes by priority, then age, so the waves of a SIMD would finish in age order and the
        // youngest walk the end of their horizons alone.  A wave in the first half of the loop's groups (`full` of them: the
        // last group of the horizon is the epilogue's, and runs at the second half's priority) outranks one in the second
        // half: the waves of a SIMD converge.  s_setprio takes an immediate, hence two copies of the loop (the
        // outer loop is unrolled).  Three copies keep the one loop: the library math (a second loop takes the goal zone's redo
        // from 80 to 82 VGPRs, a wave per SIMD), racing math = 1 (64 -> 65 VGPRs, a wave per SIMD) and the X0OUT copy, whose
        // `t == 0` test would stay inside the second loop.
        constexpr bool DRAIN = FAST != 0 && !X0OUT && !(is_racing_model(MODEL) && FAST == 1);
        ROLLOUT_TRACE_LOOP_ENTRY();
        int r = 0;
#pragma unroll
        for (int half = DRAIN ? 0 : 1; half < 2; ++half) {
            if (DRAIN && half == 0) MPPI_DRAIN_PRIO(1);
            if (DRAIN && half == 1) MPPI_DRAIN_PRIO(0);
            const int end = half == 0 ? full >> 1 : full;
            for (; r < end; ++r) {
                const int rn = min(r + 1, d.R - 1);
                const float4 en = noise_group<GEN, U1_FMA>(np, rn, gi, gen, d, &pins);  // independent chain, interleaved with the steps
                const float4 m4n = mean4[rn];
                const float ev[4] = {e.x, e.y, e.z, e.w};
                const float mv[4] = {m4.x, m4.y, m4.z, m4.w};
                float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if constexpr (AC) { const float4 gq = g4[r]; gv[0] = gq.x; gv[1] = gq.y; gv[2] = gq.z; gv[3] = gq.w; }
                if constexpr (ROLL_GROUP) {
                    rolled_group(e, m4, AC ? g4[r] : float4{0.0f, 0.0f, 0.0f, 0.0f}, false);
                } else {
#pragma unroll
                    for (int g = 0; g < SPG; ++g) one_step(ev + g * DC, mv + g * DC, gv + g * DC);
                }
                e = en;
                m4 = m4n;
            }
        }
        ROLLOUT_TRACE_LOOP_EXIT();
    } else {
        // Tiles: loads return in order (one vmcnt), so the first map gather consumed after a noise load also
        // waits for that load.  Keep two groups in flight and issue the load of group r+2 at the very END of
        // iteration r (pinned by a fake dependency on the iteration's result): it then has most of iteration r+1 to arrive.
        float4 e1 = noise_group<GEN, U1_FMA>(np, min(1, d.R - 1), gi, gen, d);
        for (int r = 0; r < full; ++r) {
            const float4 m4n = mean4[min(r + 1, d.R - 1)];
            const float ev[4] = {e.x, e.y, e.z, e.w};
            const float mv[4] = {m4.x, m4.y, m4.z, m4.w};
            float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (AC) { const float4 gq = g4[r]; gv[0] = gq.x; gv[1] = gq.y; gv[2] = gq.z; gv[3] = gq.w; }
            if constexpr (ROLL_GROUP) {
                rolled_group(e, m4, AC ? g4[r] : float4{0.0f, 0.0f, 0.0f, 0.0f}, false);
            } else {
#pragma unroll
                for (int g = 0; g < SPG; ++g) one_step(ev + g * DC, mv + g * DC, gv + g * DC);
            }
            e = e1;
            m4 = m4n;
            const float4* nptr = np + (int64_t)min(r + 2, d.R - 1) * 64;
            asm volatile("" : "+v"(nptr) : "v"(acc.a));  // the address "depends" on this iteration's last cost
            e1 = *nptr;
        }
    }
    // (One step per group, dc = 4, and no last group held back: the loops above have walked all T steps and nothing is left.  Said
    // at compile time: the compiler proved it for the 4-control learned model only while that model's step constant did not
    // carry the step index, and the dead third copy of the step cost its library-math kernels 16 VGPRs and a wave per SIMD.)
    if ((SPG > 1 || LAST_GROUP_IN_EPILOGUE || !(is_mlp(MODEL) && TRACK)) && t < d.T) {  // last group: ragged (T*dc not a multiple of 4), or, behind the regenerating loop, the complete last one
        const float ev[4] = {e.x, e.y, e.z, e.w};
        const float mv[4] = {m4.x, m4.y, m4.z, m4.w};
        float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (AC) {  // (t is a multiple of SPG here and t < T: group t / SPG < R)
            const float4 gq = g4[t / SPG];
            gv[0] = gq.x; gv[1] = gq.y; gv[2] = gq.z; gv[3] = gq.w;
        }
        if constexpr (ROLL_GROUP) {
            rolled_group(e, m4, AC ? g4[t / SPG] : float4{0.0f, 0.0f, 0.0f, 0.0f}, true);
        } else {
#pragma unroll
            for (int g = 0; g < SPG; ++g)
                if (t < d.T) one_step(ev + g * DC, mv + g * DC, gv + g * DC);
        }
    }
    // terminal cost: zero action, stale prev_action U[:, max(T-2,0)] and stale t = T-1
    // (mppi.py:318-328); knext already holds the constants of row T-1
    float zero[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) zero[k] = 0.0f;
    if constexpr (is_mlp(MODEL) && TRACK) knext = M::load_k(ktab, d.T - 1);
    float term;
    if constexpr (is_mlp(MODEL) && !TRACK) term = M::cost_plain(ctx, knext, s, zero, pl, bad);
    else term = M::cost(ctx, knext, s, zero, pl, bad);
    // The learned terminal value of the final state (mppi_set_mlp_value): launch-uniform, once per trajectory, TRACK only.  Its
    // pointer and weight come from the context, or — SLOT: the caller has parked them — from the block's LDS copy `vslot`:
    // read back here as vector values and made scalar again, so that the table is read with scalar loads either way.
    if constexpr (is_mlp(MODEL) && TRACK) {
        if constexpr (SLOT) {
            const volatile MlpValueSlot* slot = vslot;  // (volatile: read back HERE, not carried from the store in scalar registers)
            const uint64_t p = (uint64_t)slot->table;
            const uint64_t pu = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(p >> 32)) << 32;
            if (pu != 0) {
                const float w = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (float)slot->weight)));
                term = M::terminal_with_value((const float*)pu, mlp_value_flags(ctx), w, term, s);
            }
        } else if (mlp_value_on(ctx)) {
            term = M::terminal_with_value(ctx, term, s);
        }
    }
    if constexpr (AC) return action_cost_total(acc.total(term), *kappa, A);
    else return acc.total(term);
}

// Total cost of one lane's trajectory: picks the launch-uniform copy of the horizon loop (racing: unit wheel base; a start
// outside the position clamp) and — for the models whose fast paths have per-lane validity ranges (pendulum, cart-poles,
// mountain car, goal zone) — redoes a lane that left one with the library math.  Racing and nav2d take any finite start
// (EntryGeneral) and carry no redo: inlining the library-math walk next to the hot loop cost the racing kernel 18 VGPRs,
// two waves per SIMD and 3.6 % of its time (profiles/r04_experiments.md).
// AC: every copy carries the control-cost term (the redo computes its own A from scratch, like its cost sum).
template <int MODEL, int FAST, bool GEN, bool UC, bool AC = false, bool TRACK = false, bool SLOT = false>
__device__ __forceinline__ float lane_cost(const float4* __restrict__ np, uint64_t gi, const GenCtx& gen, const float4* mp,
                                           const float* s_ktab, const float* __restrict__ x0, const Dims& d,
                                           const ModelCtx& ctx, const float4* g4 = nullptr, const float* kappa = nullptr,
                                           const MlpValueSlot* vslot = nullptr) {
    using M = ModelT<MODEL, FAST>;
    bool bad = false;
    float total;
    if constexpr (FAST != 0 && EntryGeneral<M>::value) {
        if (!M::start_in_box(ctx, x0))  // launch-uniform (x0 is shared): the copy whose first stage cost is bounds-tested
            return trajectory_cost<MODEL, FAST, GEN, UC, false, true, AC>(np, gi, gen, mp, s_ktab, x0, d, ctx, bad, g4, kappa);
    }
    // (racing, fast math: the unit wheel base of the reference is a launch-uniform branch around two copies of the loop)
    if (is_racing_model(MODEL) && FAST != 0 && ctx.unit_L)
        total = trajectory_cost<MODEL, FAST, GEN, UC, true, false, AC>(np, gi, gen, mp, s_ktab, x0, d, ctx, bad, g4, kappa);
    else
        total = trajectory_cost<MODEL, FAST, GEN, UC, false, false, AC, TRACK, SLOT>(np, gi, gen, mp, s_ktab, x0, d, ctx, bad, g4, kappa, vslot);
    if constexpr (FAST != 0 && !EntryGeneral<M>::value) {
        if (bad) {  // a fast path left its validity range: redo this lane with the library math
            bool ignore = false;
            total = trajectory_cost<MODEL, 0, GEN, false, false, false, AC, TRACK, SLOT>(np, gi, gen, mp, s_ktab, x0, d, ctx, ignore, g4, kappa, vslot);
        }
    }
    return total;
}

template <int MODEL, int FAST>  // (defined with the solve's tail below)
__device__ __forceinline__ void batch1_rollout(const ModelCtx& ctx, const float* s_x0, const float* s_act, int T,
                                               float* __restrict__ state_out);

#ifndef MPPI_ROLLOUT_ATTR
#define MPPI_ROLLOUT_ATTR  // e.g. __attribute__((amdgpu_waves_per_eu(8))) for occupancy experiments
#endif

// Launch arguments of the control-cost term (rollout_action_cost_kernel, action_cost_kernel)
struct ActionCostArgs {
    const float* sigtab;      // per-column sigma [4R] (the adapted table / a wide handle's), or null: d.sigma[k]
    const float* lambda_dev;  // the temperature in device memory, or null: `lambda`
    float lambda;             // (0: no temperature yet — the term is zero)
    float weight;             // action_cost_weight
};

// rollout_cost_kernel<MODEL, FAST, GEN, UC> and, with the control-cost term (one more argument: ActionCostArgs),
// rollout_action_cost_kernel<MODEL, FAST, GEN, UC>: one text, compiled twice (mppi_rollout_kernel.inc says why).
#define MPPI_ROLLOUT_KERNEL rollout_cost_kernel
#define MPPI_ROLLOUT_AC 0
#include "mppi_rollout_kernel.inc"
#undef MPPI_ROLLOUT_KERNEL
#undef MPPI_ROLLOUT_AC
#define MPPI_ROLLOUT_KERNEL rollout_action_cost_kernel
#define MPPI_ROLLOUT_AC 1
#include "mppi_rollout_kernel.inc"
#undef MPPI_ROLLOUT_KERNEL
#undef MPPI_ROLLOUT_AC

// ------------------------------------------------------------------------------------------
// The north star's literal mapping, kept for comparison (mppi_set_option("mapping", 1)): ONE WAVEFRONT
// PER TRAJECTORY.  The wave loads the trajectory's [T*dc] noise row from the reference layout
// [N][T][dc] with coalesced float4 loads and stages U = clamp(mean + eps) in LDS; lane 0 walks the
// serial recurrence S[t+1] = f(S[t], U[t]) writing the states to LDS (63 lanes idle: the recurrence
// cannot be spread over lanes); then lane t evaluates the stage cost of step t (lane T the terminal
// cost) and a wavefront shuffle reduction sums them.  Same model functors, same results up to the
// summation order of the T+1 stage costs.  Measured 20x slower than the lane-per-trajectory mapping
//  because the recurrence runs on 1/64 of the machine.
template <int MODEL, int FAST, bool TRACK = false>
__global__ __launch_bounds__(BLOCK) void rollout_cost_wave_kernel(const float* __restrict__ eps_std,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ x0,
                                                                  float* __restrict__ costs,
                                                                  unsigned* __restrict__ min_key,
                                                                  unsigned* __restrict__ next_min_key, Dims d,
                                                                  ModelCtx ctx) {
    using M = ModelT<MODEL, FAST>;
    using K = typename M::K;
    constexpr int DS = M::DS, DC = M::DC, NW = BLOCK / WAVE;
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];  // WaveRolloutLds, per wave: U[row4] then S[(T+1)*DS]
    static_assert(NW == WaveRolloutLds::WAVES, "the launch site sizes the LDS for the block's waves");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int row4 = WaveRolloutLds::s(d.R);
    float* sU = s_dyn + (size_t)wid * (row4 + (d.T + 1) * DS);  // (WaveRolloutLds::per_wave)
    float* sS = sU + row4;
    if (blockIdx.x == 0 && threadIdx.x == 0) *next_min_key = 0xFFFFFFFFu;
    float wmin = INFINITY;
    const int64_t nwaves = (int64_t)gridDim.x * NW;
    for (int64_t i = (int64_t)blockIdx.x * NW + wid; i < d.N; i += nwaves) {
        const bool inherit = (d.sample_offset + i) < d.inherit_count;  // wave-uniform
        const float* erow = eps_std + i * d.row;
        for (int f = lane; f < d.row; f += WAVE) {  // coalesced row load, clamp, stage in LDS
            const float m = inherit ? mean[f] : 0.0f;
            sU[f] = clampf(m + erow[f], d.u_min[f % DC], d.u_max[f % DC]);
        }
        __builtin_amdgcn_wave_barrier();
        bool bad = false;
        if (lane == 0) {  // the serial recurrence: one lane
            float s[DS];
#pragma unroll
            for (int j = 0; j < DS; ++j) s[j] = x0[j];
            if (FAST) M::check_state(ctx, s, bad);
            for (int t = 0; t < d.T; ++t) {
                float u[DC], sn[DS], ss[DS];
#pragma unroll
                for (int k = 0; k < DC; ++k) u[k] = sU[t * DC + k];
                M::step(ctx, s, u, sn, ss, bad, false);
#pragma unroll
                for (int j = 0; j < DS; ++j) { sS[t * DS + j] = ss[j]; s[j] = sn[j]; }
            }
#pragma unroll
            for (int j = 0; j < DS; ++j) sS[d.T * DS + j] = s[j];
        }
        __builtin_amdgcn_wave_barrier();
        float part = 0.0f;
        for (int t = lane; t <= d.T; t += WAVE) {  // time-parallel stage costs
            float st[DS], u[DC], pu[DC];
#pragma unroll
            for (int j = 0; j < DS; ++j) st[j] = sS[t * DS + j];
            const bool term = t == d.T;
            const int tp = term ? max(d.T - 2, 0) : max(t - 1, 0);
#pragma unroll
            for (int k = 0; k < DC; ++k) { u[k] = term ? 0.0f : sU[t * DC + k]; pu[k] = sU[tp * DC + k]; }
            const K kk = M::load_k(ctx.ref, term ? d.T - 1 : t);
            if constexpr (is_mlp(MODEL) && !TRACK) {
                part += M::cost_plain(ctx, kk, st, u, pu, bad);
            } else if constexpr (is_mlp(MODEL)) {  // lane T adds the learned terminal value of the final state
                float c = M::cost(ctx, kk, st, u, pu, bad);
                if (term && mlp_value_on(ctx)) c = M::terminal_with_value(ctx, c, st);
                part += c;
            } else {
                part += M::cost(ctx, kk, st, u, pu, bad);
            }
        }
        const float total = wave_sum(part);
        if (lane == 0) { costs[i] = total; wmin = fminf(wmin, total); }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0 && wmin < INFINITY) atomicMin(min_key, float_to_key(wmin));
}

}  // namespace mppi
