// mppi_models.hpp — the five shipped dynamics/cost plugins as inlineable functors.
//
// Compiled for gfx950 by hipcc (device) and, for pre-GPU debugging only, by g++ into the test-only
// harness tests/host_emul (never loaded by the product).  All arithmetic is fp32 in the
// reference's operation order; the translation unit is built with -ffp-contract=off and fusion is
// spelled out with fmaf() where it is wanted.
//
// FAST=false uses the library sinf/cosf/tanf/fmodf and IEEE division.
// FAST=true  replaces them by branch-free fast paths that are either bit-identical (angle wrap,
//            division by the map cell size) or <=1 ulp (sin/cos/tan polynomials).  Each fast path
//            has a validity range; instead of branching to the library call inside the horizon
//            loop it raises the per-lane `bad` flag, and the caller re-runs that trajectory with
//            FAST=false after the loop (never taken for the shipped models: angles are wrapped
//            every step and the steering angle is clamped).  Preconditions that are uniform over
//            the launch (tan polynomial range, Markstein reciprocal, fused map) are checked on the
//            host, which otherwise selects the FAST=false kernel.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/mppi_hip.h"
#include "mppi_discs.hpp"

#if defined(__HIPCC__)
#define MPPI_HD __host__ __device__ __forceinline__
#else
#define MPPI_HD inline
#endif

namespace mppi {

constexpr float PI_F = 3.14159274f;      // (float)torch.pi
constexpr float TWO_PI_F = 6.28318548f;  // (float)(2*torch.pi)

struct MapView {
    const uint8_t* cells;  // [nx][ny] occupancy 0/1
    int32_t nx, ny;
    float cell, inv_cell;  // inv_cell = RN(1/cell) for the Markstein division
    float ox, oy;
};

struct ModelCtx {
    float P[MPPI_MAX_PARAMS];
    MapView maps[2];
    // FAST racing / nav2d: the occupancy grid(s) copied into one (nx+1) x (ny+1) grid whose extra row and
    // column hold the out-of-bounds value (racing: obstacle + lane summed, 0..2), addressed without any
    // bounds test (see occ_lookup_pad); `pad` is the grid's base minus the constant the index trick adds.
    const uint8_t* pad;
    int32_t pad_stride;    // ny + 1
    const float* ref;      // racing: [rows][8] = x, y, yaw, v, sin(yaw), cos(yaw), 0, 0
    int32_t ref_rows;
    int32_t tan_small;     // steer bounds within [-0.25, 0.25]: polynomial tan is valid
    float inv_L;           // racing: RN(1/L) for the Markstein division by the wheel base (0 = unusable)
    int32_t unit_L;        // racing: the wheel base is exactly 1 (the reference's value): the division disappears
    int32_t u_in_bounds;   // the solver's [u_min, u_max] lies inside the model's own action clamp
    int32_t wrap_safe;     // per-step heading increments are < pi: wrapped angles stay in the narrow range
};

// The learned-dynamics models (MPPI_MODEL_MLP41 / MLP42 with 4 states, MLP81 / MLP82 / MLP84 with 8; mppi_set_mlp): the
// weight table is ModelCtx::ref and the launch-uniform flags ride in ModelCtx::ref_rows, two fields these models have no other use for, so the kernels'
// argument struct is what it was.
constexpr int MLP_TWO_LAYERS = 1, MLP_TANH = 2, MLP_RESIDUAL = 4;
constexpr int mlp_table_floats(int dc) {
    return MPPI_MLP_HIDDEN * (4 + dc) + MPPI_MLP_HIDDEN + MPPI_MLP_HIDDEN * MPPI_MLP_HIDDEN + MPPI_MLP_HIDDEN + 4 * MPPI_MLP_HIDDEN + 4;
}
// the same table for `ds` state components: W1[H][ds + dc], b1[H], W2[H][H], b2[H], W3[ds][H], b3[ds]
constexpr int mlp_table_floats(int ds, int dc) {
    return MPPI_MLP_HIDDEN * (ds + dc) + MPPI_MLP_HIDDEN + MPPI_MLP_HIDDEN * MPPI_MLP_HIDDEN + MPPI_MLP_HIDDEN + ds * MPPI_MLP_HIDDEN + ds;
}
static_assert(mlp_table_floats(4, 1) == mlp_table_floats(1) && mlp_table_floats(4, 2) == mlp_table_floats(2) &&
              mlp_table_floats(8, 4) == 1736, "one layout for both state widths");
// the ids of the learned-dynamics models
constexpr bool is_mlp8(int model) { return model == MPPI_MODEL_MLP81 || model == MPPI_MODEL_MLP82 || model == MPPI_MODEL_MLP84; }
constexpr bool is_mlp(int model) { return model == MPPI_MODEL_MLP41 || model == MPPI_MODEL_MLP42 || is_mlp8(model); }
// A member per particle (mppi_set_particle_members; rollout_particles_kernel only): the map rides in two more fields these
// models leave free, for that one launch — ModelCtx::pad is the device table of the members' offsets into the weight buffer,
// in floats, one int32 per particle (null: no map), ModelCtx::pad_stride its length.  Read at a block-uniform index through
// the constant address space: one scalar load.
#if defined(__HIP_DEVICE_COMPILE__)
MPPI_HD const int32_t __attribute__((address_space(4)))* member_offsets(const ModelCtx& c) {
    return (const int32_t __attribute__((address_space(4)))*)c.pad;
}
#else
MPPI_HD const int32_t* member_offsets(const ModelCtx& c) { return reinterpret_cast<const int32_t*>(c.pad); }
#endif
// Tracking costs (mppi_set_mlp_reference, mppi_set_mlp_angular): the reference table [rows][2 * DS] — row t is the goal g_t[DS]
// and then the weights q_t[DS] of horizon step t — rides in one more field these models leave free, ModelCtx::maps[0].cells,
// and the mask of the angular state components in bits 8-15 of ModelCtx::ref_rows, beside the three architecture flags.  All
// zeros is "off", on the host and on the device alike: a null pointer means no reference, and goal and q come from P[] as
// before — the kernel arguments, held in scalar registers across the horizon loop as they always were; a default solver runs
// the loop it ran.  With a reference the row is read through the constant address space: where the step index is wave-uniform
// (every lane-per-trajectory kernel) the 2 * DS values are one scalar load per step, where it differs per lane
// (rollout_cost_wave_kernel) the same source compiles to per-lane loads.  mlp_flags_word composes ref_rows: its one writer on
// the host is publish_mlp_flags (capi_model.hip).
// The kernels that evaluate these models exist twice: TRACK = false is the kernel as it was (MlpModel::cost_plain: g, q of P[],
// nothing of the above in it), TRACK = true carries the tracking cost (MlpModel::cost); mlp_tracking(ctx) at the launch site
// picks one, and mlp_track(MODEL) is the template argument to ask for (false for every other model: no second instantiation).
// In the TRACK kernels the table pointer costs two scalar registers across a horizon loop that has none to spare
// (profiles/r26_mlp_tracking.md): they are won back there — no look-ahead step constant (trajectory_cost), and the
// end-of-kernel `threadIdx.x == 0` formed from the `lane == 0` mask (mppi_rollout_kernel.inc).
// A learned terminal value (mppi_set_mlp_value): a second, smaller network V(s_T) evaluated once per trajectory on its final
// state and added to (or put in place of) the terminal cost.  Its table — W1[H][DS], b1[H], W2[H][H], b2[H], w3[H], b3[1],
// unused parts zero — rides in ModelCtx::maps[1].cells, its weight in ModelCtx::maps[1].cell (a float these models leave free)
// and its three flags in bits 16-18 of ModelCtx::ref_rows.  A null pointer means no value.  It lives in the TRACK kernels only,
// behind a launch-uniform branch outside the horizon loop (trajectory_cost; lane T of rollout_cost_wave_kernel).
constexpr bool mlp_track(int model) { return is_mlp(model); }
constexpr int MLP_ARCH_MASK = MLP_TWO_LAYERS | MLP_TANH | MLP_RESIDUAL, MLP_ANGULAR_SHIFT = 8, MLP_VALUE_SHIFT = 16;
constexpr int MLP_VALUE_TWO_LAYERS = 1, MLP_VALUE_TANH = 2, MLP_VALUE_REPLACE = 4, MLP_VALUE_MASK = 7;  // (as shifted down)
constexpr int mlp_value_floats(int ds) {
    return MPPI_MLP_HIDDEN * ds + MPPI_MLP_HIDDEN + MPPI_MLP_HIDDEN * MPPI_MLP_HIDDEN + MPPI_MLP_HIDDEN + MPPI_MLP_HIDDEN + 1;
}
constexpr int32_t mlp_flags_word(int arch, uint32_t angular, int value = 0) {
    return (int32_t)((uint32_t)(arch & MLP_ARCH_MASK) | ((angular & 0xffu) << MLP_ANGULAR_SHIFT) |
                     ((uint32_t)(value & MLP_VALUE_MASK) << MLP_VALUE_SHIFT));
}
MPPI_HD int mlp_value_flags(const ModelCtx& c) { return (int)(((uint32_t)c.ref_rows >> MLP_VALUE_SHIFT) & (uint32_t)MLP_VALUE_MASK); }
MPPI_HD bool mlp_value_on(const ModelCtx& c) { return c.maps[1].cells != nullptr; }  // (launch-uniform)
MPPI_HD float mlp_value_weight(const ModelCtx& c) { return c.maps[1].cell; }
// A block's LDS copy of the value's pointer and weight: the rollout kernels park the two there across the horizon loop, which
// has no scalar registers to spare for them (mppi_rollout_kernel.inc), and trajectory_cost reads them back behind the loop.
struct MlpValueSlot { const float* table; float weight; int64_t n; };  // (n: the kernel's sample count, which waits there too)
inline void set_mlp_value(ModelCtx& c, const float* table, float weight) {
    c.maps[1].cells = reinterpret_cast<const uint8_t*>(table);
    c.maps[1].cell = table ? weight : 0.0f;
}
MPPI_HD uint32_t mlp_angular(const ModelCtx& c) { return ((uint32_t)c.ref_rows >> MLP_ANGULAR_SHIFT) & 0xffu; }
#if defined(__HIP_DEVICE_COMPILE__)
MPPI_HD const float __attribute__((address_space(4)))* mlp_reference(const ModelCtx& c) {
    return (const float __attribute__((address_space(4)))*)c.maps[0].cells;
}
#else
MPPI_HD const float* mlp_reference(const ModelCtx& c) { return reinterpret_cast<const float*>(c.maps[0].cells); }
#endif
MPPI_HD bool mlp_tracking(const ModelCtx& c) {  // (launch-uniform: a reference, a mask or a terminal value)
    return c.maps[0].cells != nullptr || mlp_angular(c) != 0 || mlp_value_on(c);
}
inline void set_mlp_reference(ModelCtx& c, const float* table) { c.maps[0].cells = reinterpret_cast<const uint8_t*>(table); }
constexpr float MLP_TWO_PI = 6.2831855f, MLP_INV_TWO_PI = 0.15915494f;  // the wrap of an angular error: d - TWO_PI * rint(d * INV_TWO_PI)

// The step table: the models whose cost reads step-constant values carry ONE table with one row per horizon step.  It is
// ModelCtx::ref, ref_rows is the number of rows every part of it covers (the solve checks it against the horizon), and the
// rollout kernels stage T rows of it into LDS.  A row has up to two parts, each with a writer of its own on the host:
//   the reference part   racing's reference row in floats [0, ref_floats)         (mppi_set_reference / mppi_ref_window)
//   the disc part        MPPI_MAX_DISCS padded discs {cx, cy, r2, w} in floats [disc_off, disc_off + DISC_ROW), each disc
//                        16-byte aligned                                           (mppi_set_discs)
// step_layout(model) says which floats of a row belong to whom; the functors' KROW is its stride (asserted at the end of
// this file).  The launch-uniform number of discs per row rides where the model has a free field, so that the kernels'
// argument struct is what it was: nav2d with discs in ModelCtx::tan_small (a racing flag), racing with discs in the first
// P[] slot behind racing's parameters, as the BITS of the integer (no conversion on the device; mppi_set_model_params
// writes MPPI_RP_COUNT values and leaves it alone).
static_assert(DISC_ROW == 4 * MPPI_MAX_DISCS, "mppi_discs.hpp spells the row of MPPI_MAX_DISCS discs");
constexpr int RACING_REF_ROW = 8;                            // floats of a racing reference row
constexpr int RACING_DISCS_KROW = RACING_REF_ROW + DISC_ROW;  // 40
constexpr int RACING_DISCS_SLOT = MPPI_RP_COUNT;              // P[] slot of the disc count
static_assert(RACING_DISCS_SLOT < MPPI_MAX_PARAMS, "the disc count needs a free parameter slot");
constexpr bool is_racing_model(int model) {
    return model == MPPI_MODEL_RACING || model == MPPI_MODEL_RACING_DISCS || model == MPPI_MODEL_RACING_DISCS_SOFT;
}
// the soft disc models (mppi_set_disc_softness): the hard models' table, staging and count, a graded skirt in the cost
constexpr bool is_soft_discs(int model) { return model == MPPI_MODEL_NAV2D_DISCS_SOFT || model == MPPI_MODEL_RACING_DISCS_SOFT; }
struct StepLayout {
    int stride;      // floats per step row (0: the model has no step table)
    int ref_floats;  // the reference part is floats [0, ref_floats) (0: none)
    int disc_off;    // the disc part starts at this float (-1: none)
    constexpr bool has_ref() const { return ref_floats > 0; }
    constexpr bool has_discs() const { return disc_off >= 0; }
};
constexpr StepLayout step_layout(int model) {
    return model == MPPI_MODEL_RACING         ? StepLayout{RACING_REF_ROW, RACING_REF_ROW, -1}
           : model == MPPI_MODEL_NAV2D_DISCS  ? StepLayout{DISC_ROW, 0, 0}
           : model == MPPI_MODEL_RACING_DISCS ? StepLayout{RACING_DISCS_KROW, RACING_REF_ROW, RACING_REF_ROW}
           : model == MPPI_MODEL_NAV2D_DISCS_SOFT  ? StepLayout{DISC_ROW, 0, 0}
           : model == MPPI_MODEL_RACING_DISCS_SOFT ? StepLayout{RACING_DISCS_KROW, RACING_REF_ROW, RACING_REF_ROW}
                                              : StepLayout{0, 0, -1};
}
static_assert(step_layout(MPPI_MODEL_RACING_DISCS).disc_off % 4 == 0 && step_layout(MPPI_MODEL_RACING_DISCS).stride % 4 == 0,
              "discs stay 16-byte aligned behind the reference row");
// the models that carry a disc table (mppi_set_discs)
constexpr bool has_discs(int model) { return step_layout(model).has_discs(); }
// the descriptor's two fields under the names the host programs of the tests read them by
constexpr int ref_stride(int model) { return step_layout(model).stride; }
constexpr int disc_offset(int model) { return step_layout(model).disc_off; }
// The number of discs per row: the one accessor both disc models go through (`model`: a constant where a kernel calls it)
MPPI_HD int disc_count(const ModelCtx& c, int model = MPPI_MODEL_NAV2D_DISCS) {
    if (!is_racing_model(model)) return c.tan_small;
    int32_t n;
    __builtin_memcpy(&n, &c.P[RACING_DISCS_SLOT], sizeof(n));
    return n;
}
inline void set_disc_count(ModelCtx& c, int model, int n) {
    if (!is_racing_model(model)) { c.tan_small = n; return; }
    const int32_t v = n;
    __builtin_memcpy(&c.P[RACING_DISCS_SLOT], &v, sizeof(v));
}
// The two coefficients {a, b} of the soft rule (mppi_discs.hpp) ride in free P[] slots too, which mppi_set_model_params does
// not write: behind nav2d's parameters, and behind racing's disc count
constexpr int soft_slot(int model) { return is_racing_model(model) ? RACING_DISCS_SLOT + 1 : MPPI_NP_COUNT; }
static_assert(soft_slot(MPPI_MODEL_NAV2D_DISCS_SOFT) + 1 < MPPI_MAX_PARAMS && soft_slot(MPPI_MODEL_RACING_DISCS_SOFT) + 1 < MPPI_MAX_PARAMS,
              "the soft coefficients need two free parameter slots");
struct DiscSoft { float a, b; };
MPPI_HD DiscSoft disc_soft(const ModelCtx& c, int model) { return DiscSoft{c.P[soft_slot(model)], c.P[soft_slot(model) + 1]}; }
inline void set_disc_soft(ModelCtx& c, int model, float a, float b) { c.P[soft_slot(model)] = a; c.P[soft_slot(model) + 1] = b; }

// Host-side plan of the padded grid.  The models clamp positions to [xlo, xhi] x [ylo, yhi]; if every index
// round(p/cell + origin) reachable under that clamp lies in [0, nx] x [0, ny], the lookup needs no bounds test.
// koff = the constant (mod 2^32) that occ_lookup_pad's index carries; returns false when the plan does not apply.
inline bool pad_map_plan(const MapView& m, float xlo, float xhi, float ylo, float yhi, uint32_t& koff) {
    if (!(m.cell > 0.0f) || m.nx < 1 || m.ny < 1 || m.nx >= (1 << 20) || m.ny >= (1 << 20)) return false;
    const float ix0 = rintf(xlo / m.cell + m.ox), ix1 = rintf(xhi / m.cell + m.ox);  // IEEE division = the
    const float iy0 = rintf(ylo / m.cell + m.oy), iy1 = rintf(yhi / m.cell + m.oy);  // device's Markstein quotient
    if (!(ix0 >= 0.0f && ix1 <= (float)m.nx && iy0 >= 0.0f && iy1 <= (float)m.ny)) return false;
    const uint64_t k = 0x400000ull * (uint64_t)(m.ny + 1) + 0x4B400000ull;
    koff = (uint32_t)k;
    return (uint64_t)koff + (uint64_t)(m.nx + 1) * (uint64_t)(m.ny + 1) < (1ull << 32);
}

// torch.clamp(x, lo, hi) = min(max(x, lo), hi).  On the device this is one v_med3_f32 (identical for
// lo <= hi and non-NaN x; NaN inputs are outside the contract).
MPPI_HD float clampf(float x, float lo, float hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(x, lo, hi);
#else
    return fminf(fmaxf(x, lo), hi);
#endif
}

// Total cost of a trajectory = sum_t stage cost + terminal cost (mppi.py:333-334: torch.sum(costs, dim=1) + terminal).
// The order of torch.sum is not part of the reference's contract (a vectorised cascade on the CPU that depends on the
// ISA, a tree on a GPU), and softmax(-c / lambda) amplifies the last bits of c by |c| / lambda: the reference's own
// action sequence moves by 2e-5 .. 7e-5 (nav2d, goal zone at lambda = 1) when its costs are re-summed in another valid
// fp32 order (tests/golden/make_golden.py: the recorded bands).  EXACT = true adds the fp32 stage costs in DOUBLE and
// rounds once: the value every fp32 order approximates, so the distance to ANY build of the reference is that build's own
// rounding error only (the sequential fp32 sum of rounds 1-3 sat at the edge of the reference's spread: 2.7e-5 against a
// band of 2.7e-5 on nav2d).  EXACT = false is the plain sequential fp32 sum, kept for racing: its costs / lambda are
// far from that regime (an arg-min at lambda = 1, 1e4-scale obstacle costs over lambda >= 100 in the dense cases: the
// reference's own spread is <= 6e-6 and the kernel's distance to it <= 2e-6), and in its VALU-issue-bound kernel the
// conversion + half-rate add + register-pair moves are 6 of 209 instructions per two steps: 125.1 against 121.7 us
// (profiles/r04_experiments.md).
template <bool EXACT>
struct CostSum {
    float a = 0.0f;
    MPPI_HD void add(float c) { a += c; }
    MPPI_HD float total(float terminal) const { return a + terminal; }
};
template <>
struct CostSum<true> {
    double a = 0.0;
    MPPI_HD void add(float c) { a += (double)c; }
    MPPI_HD float total(float terminal) const { return (float)(a + (double)terminal); }
};
#ifndef MPPI_EXACT_SUM_RACING
#define MPPI_EXACT_SUM_RACING 0  // (A/B knob of scripts/build_variant.sh: the double accumulator in the racing kernel too)
#endif
constexpr bool exact_cost_sum(int model) { return MPPI_EXACT_SUM_RACING || !is_racing_model(model); }

}  // namespace mppi

// The model code is compiled twice:
//   mppi::strict — FP contraction off: every multiply and add rounds separately, in the reference's
//                  (unfused torch) operation order.  Used with FAST=false (library math).
//   mppi::fused  — FP contraction on: a*b+c may become one FMA (one rounding instead of two).  Used with
//                  FAST=true, whose sin/cos/tan already differ from the library math by <= 1.5 ulp; the
//                  fused form saves ~13 VALU instructions per racing step.  Parity tests bound both
//                  against the oracle at 1e-5.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#define MPPI_MODEL_NS strict
#define MPPI_MODEL_HWTRIG false
#include "mppi_models.inc"
#undef MPPI_MODEL_NS
#undef MPPI_MODEL_HWTRIG
//   mppi::fused_hw — as mppi::fused, with sin/cos of arguments the MODEL bounds — the wrapped headings of the kinematic
//                  models (racing, nav2d, goal zone: the `CHECK = false` call sites of sincos_f, argument in [-pi, pi))
//                  and the clamped pole angle / position of the cart-pole and the mountain car (sincos_b, |x| <= 4
//                  or the lane is redone) — evaluated by the hardware v_sin_f32 / v_cos_f32 (argument in revolutions):
//                  measured max abs error 2.7e-7 against 7.8e-8 of the polynomials (scripts/ubench/hw_sincos_acc.hip)
//                  — below half an ulp of any position beyond 4 m — for 3 instead of 24 instructions per step.
//                  The pendulum's free angle and the MuJoCo-style cart-pole keep the exactly reduced polynomials.
//                  Device only.
#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
#define MPPI_MODEL_NS fused
#define MPPI_MODEL_HWTRIG false
#include "mppi_models.inc"
#undef MPPI_MODEL_NS
#undef MPPI_MODEL_HWTRIG
#if defined(__HIPCC__)
#define MPPI_MODEL_NS fused_hw
#define MPPI_MODEL_HWTRIG true
#include "mppi_models.inc"
#undef MPPI_MODEL_NS
#undef MPPI_MODEL_HWTRIG
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mppi {
// The math level selects the functor: 0 = library math, unfused (the reference's operation order);
// 1 = range-checked fast paths, fused; 2 = level 1 + hardware sin/cos for the wrapped headings.
template <int MODEL, int MATH>
struct ModelSel { using type = strict::Model<MODEL, false>; };
template <int MODEL>
struct ModelSel<MODEL, 1> { using type = fused::Model<MODEL, true>; };
#if defined(__HIPCC__)
template <int MODEL>
struct ModelSel<MODEL, 2> { using type = fused_hw::Model<MODEL, true>; };
#endif
template <int MODEL, int MATH>
using ModelT = typename ModelSel<MODEL, MATH>::type;

// Models whose fast-math cost loop takes ANY finite initial state (Model::enter_any / start_in_box / cost(..., general)):
// no lane of theirs can leave a fast path's validity range, so their cost kernels carry no library-math redo.
template <class M, class = void>
struct EntryGeneral { static constexpr bool value = false; };
template <class M>
struct EntryGeneral<M, decltype((void)M::ENTRY_GENERAL)> { static constexpr bool value = M::ENTRY_GENERAL; };

// every functor stages the row its model's step layout describes
template <int MODEL>
constexpr bool krow_is_stride() { return ModelT<MODEL, 0>::KROW == step_layout(MODEL).stride; }
static_assert(krow_is_stride<MPPI_MODEL_PENDULUM>() && krow_is_stride<MPPI_MODEL_CARTPOLE>() && krow_is_stride<MPPI_MODEL_MOUNTAINCAR>() &&
              krow_is_stride<MPPI_MODEL_NAV2D>() && krow_is_stride<MPPI_MODEL_RACING>() && krow_is_stride<MPPI_MODEL_MJCARTPOLE>() &&
              krow_is_stride<MPPI_MODEL_GOALZONE>() && krow_is_stride<MPPI_MODEL_MLP41>() && krow_is_stride<MPPI_MODEL_MLP42>() &&
              krow_is_stride<MPPI_MODEL_NAV2D_DISCS>() && krow_is_stride<MPPI_MODEL_RACING_DISCS>() &&
              krow_is_stride<MPPI_MODEL_NAV2D_DISCS_SOFT>() && krow_is_stride<MPPI_MODEL_RACING_DISCS_SOFT>() &&
              krow_is_stride<MPPI_MODEL_MLP81>() && krow_is_stride<MPPI_MODEL_MLP82>() && krow_is_stride<MPPI_MODEL_MLP84>(),
              "a functor's KROW is the stride of step_layout(model)");
}  // namespace mppi
