// Host build of the product's model functors (mppi_playground_amd/csrc/mppi_models.hpp) for
// pre-GPU debugging of the model math, both FAST variants.  TEST-ONLY: the product never loads this
// library; it exists so that tests can compare the device functors' arithmetic with the oracle on
// a machine without a GPU.  The trajectory walk mirrors trajectory_cost() in mppi_rollout.hpp but
// reads the reference layout eps[N][T][dc].
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../mppi_playground_amd/csrc/mppi_models.hpp"

using namespace mppi;

// The kernel's entry (trajectory_cost / lane_cost in mppi_rollout.hpp): models with EntryGeneral wrap any finite heading
// once with the reference's operation and, when the start lies outside the position clamp, take the bounds-tested lookup
// for the stage cost of step 0; the other models range-check the state (a bad lane is redone with the library math).
template <int MODEL, bool FAST>
static float walk(const float* eps_row, const float* mean, const float* x0, int T, const float* umin,
                  const float* umax, const ModelCtx& ctx, bool inherit, bool& bad, float* S_out) {
    using M = ModelT<MODEL, FAST>;
    constexpr int DS = M::DS, DC = M::DC;
    float s[DS], pu[DC], pl[DC];
    for (int j = 0; j < DS; ++j) s[j] = x0[j];
    bool x0_out = false;
    float raw_heading = 0.f;
    if constexpr (FAST && EntryGeneral<M>::value) {
        x0_out = !M::start_in_box(ctx, s);
        raw_heading = s[2];
        M::enter_any(s);
    } else if (FAST) {
        M::check_state(ctx, s, bad);
    }
    for (int k = 0; k < DC; ++k) pu[k] = pl[k] = 0.f;
    CostSum<exact_cost_sum(MODEL)> acc;
    for (int t = 0; t < T; ++t) {
        float u[DC], sn[DS], ss[DS];
        for (int k = 0; k < DC; ++k) {
            const float m = inherit ? mean[t * DC + k] : 0.0f;
            u[k] = clampf(m + eps_row[t * DC + k], umin[k], umax[k]);
        }
        if (t == 0) for (int k = 0; k < DC; ++k) pu[k] = u[k];
        if constexpr (FAST && EntryGeneral<M>::value) {
            M::step(ctx, s, u, sn, ss, bad, ctx.u_in_bounds != 0, true);  // (the heading entered the loop wrapped)
            acc.add(M::cost(ctx, M::load_k(ctx.ref, t), ss, u, pu, bad, x0_out && t == 0));
            if (t == 0) ss[2] = raw_heading;  // (what the reference leaves in S[:, 0]: the caller's heading as given)
        } else {
            M::step(ctx, s, u, sn, ss, bad, ctx.u_in_bounds != 0);
            acc.add(M::cost(ctx, M::load_k(ctx.ref, t), ss, u, pu, bad));
        }
        for (int k = 0; k < DC; ++k) { pl[k] = pu[k]; pu[k] = u[k]; }
        for (int j = 0; j < DS; ++j) { if (S_out) S_out[t * DS + j] = ss[j]; s[j] = sn[j]; }
    }
    for (int j = 0; j < DS; ++j) if (S_out) S_out[T * DS + j] = s[j];
    float zero[DC];
    for (int k = 0; k < DC; ++k) zero[k] = 0.f;
    return acc.total(M::cost(ctx, M::load_k(ctx.ref, T - 1), s, zero, pl, bad));
}

template <int MODEL>
static void run(int fast, int N, int T, int threshold, const float* x0, const float* mean, const float* eps,
                const float* umin, const float* umax, const ModelCtx& ctx, float* costs, uint8_t* bad_out,
                float* S_out) {
    constexpr int DS = ModelT<MODEL, false>::DS, DC = ModelT<MODEL, false>::DC;
    for (int i = 0; i < N; ++i) {
        bool bad = false;
        float* So = S_out ? S_out + (size_t)i * (T + 1) * DS : nullptr;
        const float* row = eps + (size_t)i * T * DC;
        float c = fast ? walk<MODEL, true>(row, mean, x0, T, umin, umax, ctx, i < threshold, bad, So)
                       : walk<MODEL, false>(row, mean, x0, T, umin, umax, ctx, i < threshold, bad, So);
        if (bad_out) bad_out[i] = bad ? 1 : 0;
        if (fast && bad) { bool ig = false; c = walk<MODEL, false>(row, mean, x0, T, umin, umax, ctx, i < threshold, ig, So); }
        costs[i] = c;
    }
}

extern "C" {

// maps: cells pointers + geometry as flat arrays; ref [rows][4]
int emul_rollout_cost(int model, int fast, int N, int T, int threshold, const float* x0, const float* mean,
                      const float* eps, const float* umin, const float* umax, const float* params, int nparams,
                      const uint8_t* map0, const uint8_t* map1, const int* map_dims /*nx,ny*/,
                      const float* map_geom /*cell,ox,oy*/, const float* ref, int ref_rows, float* costs,
                      uint8_t* bad_out, float* S_out) {
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    for (int i = 0; i < nparams; ++i) ctx.P[i] = params[i];
    std::vector<uint8_t> fused;
    std::vector<float> ref8;
    const uint8_t* mp[2] = {map0, map1};
    for (int sidx = 0; sidx < 2; ++sidx) if (mp[sidx]) {
        MapView& m = ctx.maps[sidx];
        m.cells = mp[sidx]; m.nx = map_dims[0]; m.ny = map_dims[1];
        m.cell = map_geom[0]; m.inv_cell = 1.0f / m.cell; m.ox = map_geom[1]; m.oy = map_geom[2];
    }
    if (map0 && (model == MPPI_MODEL_RACING ? map1 != nullptr : model == MPPI_MODEL_NAV2D)) {
        // the padded grid of the FAST lookup, planned exactly like the C ABI does (pad_map_plan)
        const bool racing = model == MPPI_MODEL_RACING;
        const float* P = ctx.P;
        const float xlo = P[racing ? MPPI_RP_XLO : MPPI_NP_XLO], xhi = P[racing ? MPPI_RP_XHI : MPPI_NP_XHI];
        const float ylo = P[racing ? MPPI_RP_YLO : MPPI_NP_YLO], yhi = P[racing ? MPPI_RP_YHI : MPPI_NP_YHI];
        uint32_t koff = 0;
        if (!pad_map_plan(ctx.maps[0], xlo, xhi, ylo, yhi, koff)) return -2;
        const int nx = map_dims[0], ny = map_dims[1];
        fused.assign((size_t)(nx + 1) * (ny + 1), racing ? 2 : 1);
        for (int ix = 0; ix < nx; ++ix)
            for (int iy = 0; iy < ny; ++iy)
                fused[(size_t)ix * (ny + 1) + iy] = map0[(size_t)ix * ny + iy] + (racing ? map1[(size_t)ix * ny + iy] : 0);
        ctx.pad = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(fused.data()) - (uintptr_t)koff);
        ctx.pad_stride = ny + 1;
    }
    if (ref) {
        ref8.resize((size_t)ref_rows * 8);
        for (int i = 0; i < ref_rows; ++i) {
            float* o = &ref8[(size_t)i * 8];
            o[0] = ref[4 * i]; o[1] = ref[4 * i + 1]; o[2] = ref[4 * i + 2]; o[3] = ref[4 * i + 3];
            o[4] = sinf(o[2]); o[5] = cosf(o[2]); o[6] = o[7] = 0.f;
        }
        ctx.ref = ref8.data(); ctx.ref_rows = ref_rows;
    }
    if (model == MPPI_MODEL_RACING) { ctx.tan_small = 1; ctx.inv_L = 1.0f / ctx.P[MPPI_RP_L]; }
    ctx.u_in_bounds = 1; ctx.wrap_safe = 1;  // the shipped parameter sets satisfy both (checked by the C ABI on the device path)
    switch (model) {
    case MPPI_MODEL_PENDULUM: run<MPPI_MODEL_PENDULUM>(fast, N, T, threshold, x0, mean, eps, umin, umax, ctx, costs, bad_out, S_out); break;
    case MPPI_MODEL_CARTPOLE: run<MPPI_MODEL_CARTPOLE>(fast, N, T, threshold, x0, mean, eps, umin, umax, ctx, costs, bad_out, S_out); break;
    case MPPI_MODEL_MOUNTAINCAR: run<MPPI_MODEL_MOUNTAINCAR>(fast, N, T, threshold, x0, mean, eps, umin, umax, ctx, costs, bad_out, S_out); break;
    case MPPI_MODEL_NAV2D: run<MPPI_MODEL_NAV2D>(fast, N, T, threshold, x0, mean, eps, umin, umax, ctx, costs, bad_out, S_out); break;
    case MPPI_MODEL_RACING: run<MPPI_MODEL_RACING>(fast, N, T, threshold, x0, mean, eps, umin, umax, ctx, costs, bad_out, S_out); break;
    case MPPI_MODEL_MJCARTPOLE: run<MPPI_MODEL_MJCARTPOLE>(fast, N, T, threshold, x0, mean, eps, umin, umax, ctx, costs, bad_out, S_out); break;
    case MPPI_MODEL_GOALZONE: run<MPPI_MODEL_GOALZONE>(fast, N, T, threshold, x0, mean, eps, umin, umax, ctx, costs, bad_out, S_out); break;
    default: return -1;
    }
    return 0;
}

// The map lookups of the nav2d / racing cost kernels on one geometry (tests/lookup_cases.py), each as the header defines it:
// the plan of the padded grid for the position limits lim = {xlo, xhi, ylo, yhi} (pad_map_plan: verdict and koff), the padded
// lookup on a grid built the way pad_map_kernel builds it (map1: racing's lane grid, summed in; ring = 1 or 2) and addressed
// through a base pointer koff below it as refresh_pad leaves it, and the bounds-tested lookup with Markstein's and with the
// IEEE quotient.  inv_cell is prepare_map's (0 for a cell size whose significand is all ones: no fast lookups then).
// Returns bit 0: the plan is accepted, bit 1: inv_cell is usable.  pad_out is written (else -1) for the points inside the
// limits when both hold — the only ones the kernels hand to occ_lookup_pad — and fast_out (else -1) when bit 1 holds.
int emul_map_lookup(const uint8_t* map0, const uint8_t* map1, int nx, int ny, float cell, float ox, float oy, const float* lim,
                    const float* pts, int64_t n, uint32_t* koff_out, float* pad_out, float* fast_out, float* lib_out) {
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    const uint8_t* mp[2] = {map0, map1};
    uint32_t bits; std::memcpy(&bits, &cell, 4);
    const bool all_ones = (bits & 0x7fffffu) == 0x7fffffu;
    for (int sidx = 0; sidx < 2; ++sidx) {
        MapView& m = ctx.maps[sidx];
        m.cells = mp[sidx]; m.nx = nx; m.ny = ny; m.cell = cell; m.ox = ox; m.oy = oy;
        m.inv_cell = all_ones ? 0.0f : 1.0f / cell;
    }
    uint32_t koff = 0;
    const bool plan = pad_map_plan(ctx.maps[0], lim[0], lim[1], lim[2], lim[3], koff);
    if (koff_out) *koff_out = koff;
    std::vector<uint8_t> pad;
    const bool padded = plan && !all_ones;
    if (padded) {
        pad.resize((size_t)(nx + 1) * (ny + 1));
        for (int ix = 0; ix <= nx; ++ix)
            for (int iy = 0; iy <= ny; ++iy) {  // one thread of pad_map_kernel
                uint8_t v = map1 ? 2 : 1;
                if (ix < nx && iy < ny) {
                    v = map0[(size_t)ix * ny + iy];
                    if (map1) v = (uint8_t)(v + map1[(size_t)ix * ny + iy]);
                }
                pad[(size_t)ix * (ny + 1) + iy] = v;
            }
        ctx.pad = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(pad.data()) - (uintptr_t)koff);
        ctx.pad_stride = ny + 1;
    }
    for (int64_t i = 0; i < n; ++i) {
        const float px = pts[2 * i], py = pts[2 * i + 1];
        const bool inside = px >= lim[0] && px <= lim[1] && py >= lim[2] && py <= lim[3];
        pad_out[i] = padded && inside ? mppi::strict::occ_lookup_pad(ctx, ctx.maps[0], px, py) : -1.0f;
        float f = -1.0f, l = 0.0f;
        for (int sidx = 0; sidx < (map1 ? 2 : 1); ++sidx) {
            const MapView& m = ctx.maps[sidx];
            if (!all_ones) f = (sidx ? f : 0.0f) + mppi::strict::occ_lookup<true>(m, m.cells, px, py, 1.0f);
            l += mppi::strict::occ_lookup<false>(m, m.cells, px, py, 1.0f);
        }
        fast_out[i] = f;
        lib_out[i] = l;
    }
    return (plan ? 1 : 0) | (all_ones ? 0 : 2);
}

// element-wise pins of the fast math against the library math
using namespace mppi::strict;  // element-wise pins: same functions in both contraction variants
void emul_sincos(const float* x, float* s, float* c, int n, int fast) {
    for (int i = 0; i < n; ++i) { bool b = false; if (fast) sincos_f<true>(x[i], s[i], c[i], b); else sincos_f<false>(x[i], s[i], c[i], b); }
}
// in-loop wraps of the kinematic models against the library wrap: mode 0 rewrap_f, 1 wrap_inc_f
void emul_loop_wraps(const float* x, float* fast_out, float* lib_out, int n, int mode) {
    for (int i = 0; i < n; ++i) {
        bool b = false;
        fast_out[i] = mode == 0 ? rewrap_f(x[i]) : wrap_inc_f(x[i]);
        lib_out[i] = angle_normalize<false>(x[i], b);
    }
}
void emul_angle_normalize(const float* x, float* y, uint8_t* bad, int n, int mode /*0 lib,1 narrow,2 wide*/) {
    for (int i = 0; i < n; ++i) {
        bool b = false;
        y[i] = mode == 0 ? angle_normalize<false>(x[i], b) : mode == 1 ? angle_normalize<true, false>(x[i], b) : angle_normalize<true, true>(x[i], b);
        bad[i] = b;
    }
}
void emul_tan(const float* x, float* y, int n, int fast) {
    for (int i = 0; i < n; ++i) y[i] = fast ? tan_f<true>(x[i]) : tan_f<false>(x[i]);
}
void emul_div_cell(const float* x, float* y, int n, float cell, int fast) {
    MapView m{}; m.cell = cell; m.inv_cell = 1.0f / cell;
    for (int i = 0; i < n; ++i) y[i] = fast ? div_cell<true>(x[i], m) : div_cell<false>(x[i], m);
}
}
