// Host build of the two soft-disc functors (Model<MPPI_MODEL_NAV2D_DISCS_SOFT> and Model<MPPI_MODEL_RACING_DISCS_SOFT> of
// mppi_playground_amd/csrc/mppi_models.inc, the arithmetic of csrc/mppi_discs.hpp) for tests/test_soft_discs_host.py.
// TEST-ONLY: the product never loads this.  Built twice from this one text:
//   as a shared library (ctypes: soft_discs_emul_nav2d, soft_discs_emul_racing, soft_discs_emul_facts), and
//   with -DSOFT_DISCS_EMUL_MAIN -fsanitize=address,undefined as a stand-alone program: `soft_discs_emul_main cases.bin
//   costs.bin` walks the cases the test wrote (per case: int32 {racing, fast, kind, N, T, rows, n, nx, ny}, float32 {a, b}, then
//   the 12 / 17 parameters, {cell, ox, oy}, the one / two nx * ny maps, racing only: the reference rows [rows][8], the PADDED
//   discs [rows][8][4], x0[3 / 4] and U[N][T][2] as float32) in heap buffers of exactly those sizes — a read past a table row or
//   an action row is a sanitizer report — and writes the costs.
// kind: 0 = the soft functor with the coefficients {a, b}, 1 = the hard disc functor, 2 = plain nav2d / racing on the same
// inputs.  The walks are those of discs_emul.cpp and racing_discs_emul.cpp (trajectory_cost() of mppi_rollout.hpp on actions
// the caller has already clamped): the stage cost of step t reads row t, the terminal cost row T-1.  Level 1 uses the
// bounds-tested map lookups (`general`).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mppi_playground_amd/csrc/mppi_models.hpp"

using namespace mppi;

// RACING: info["prev_action"] of step 0 is U[0] itself, the terminal cost sees the stale U[max(T-2, 0)], and the recorded state
// of step 0 is the start itself (heading unwrapped); nav2d's cost reads no action
template <int MODEL, bool FAST, bool RACING>
static void walk(const ModelCtx& ctx, const float* x0, const float* U, int N, int T, float* costs, float* S_out) {
    using M = ModelT<MODEL, FAST ? 1 : 0>;
    constexpr int DS = M::DS, DC = M::DC;
    for (int i = 0; i < N; ++i) {
        const float* Ui = U + (size_t)i * T * DC;
        float s[DS], zero[DC], pu[DC], pl[DC];
        bool bad = false;
        for (int j = 0; j < DS; ++j) s[j] = x0[j];
        if (FAST) M::enter_any(s);
        for (int k = 0; k < DC; ++k) { zero[k] = 0.0f; pu[k] = pl[k] = RACING ? Ui[k] : 0.0f; }
        CostSum<exact_cost_sum(MODEL)> acc;
        for (int t = 0; t < T; ++t) {
            const float* u = Ui + (size_t)t * DC;
            float sn[DS], ss[DS];
            M::step(ctx, s, u, sn, ss, bad, false, FAST);
            acc.add(M::cost(ctx, M::load_k(ctx.ref, t), ss, u, pu, bad, true));
            if (RACING)
                for (int k = 0; k < DC; ++k) { pl[k] = pu[k]; pu[k] = u[k]; }
            for (int j = 0; j < DS; ++j) {
                if (S_out) S_out[((size_t)i * (T + 1) + t) * DS + j] = (RACING && t == 0 ? x0[j] : ss[j]);
                s[j] = sn[j];
            }
        }
        for (int j = 0; j < DS; ++j)
            if (S_out) S_out[((size_t)i * (T + 1) + T) * DS + j] = s[j];
        costs[i] = acc.total(M::cost(ctx, M::load_k(ctx.ref, T - 1), s, zero, pl, bad, true));
        if (bad) costs[i] = NAN;  // (never taken: the entry is general)
    }
}

template <int MODEL, bool RACING>
static void walk_level(int fast, const ModelCtx& ctx, const float* x0, const float* U, int N, int T, float* costs, float* S_out) {
    if (fast) walk<MODEL, true, RACING>(ctx, x0, U, N, T, costs, S_out);
    else walk<MODEL, false, RACING>(ctx, x0, U, N, T, costs, S_out);
}

// {id of the nav2d model, id of the racing model, KROW of each, P[] slot of the first coefficient of each, P[] slot of the
//  racing disc count, sequential cost sum (1) or the double accumulator (0) of each}
extern "C" void soft_discs_emul_facts(int* out) {
    out[0] = MPPI_MODEL_NAV2D_DISCS_SOFT;
    out[1] = MPPI_MODEL_RACING_DISCS_SOFT;
    out[2] = ModelT<MPPI_MODEL_NAV2D_DISCS_SOFT, 0>::KROW;
    out[3] = ModelT<MPPI_MODEL_RACING_DISCS_SOFT, 0>::KROW;
    out[4] = soft_slot(MPPI_MODEL_NAV2D_DISCS_SOFT);
    out[5] = soft_slot(MPPI_MODEL_RACING_DISCS_SOFT);
    out[6] = RACING_DISCS_SLOT;
    out[7] = exact_cost_sum(MPPI_MODEL_NAV2D_DISCS_SOFT) ? 0 : 1;
    out[8] = exact_cost_sum(MPPI_MODEL_RACING_DISCS_SOFT) ? 0 : 1;
    out[9] = (is_soft_discs(MPPI_MODEL_NAV2D_DISCS_SOFT) && is_soft_discs(MPPI_MODEL_RACING_DISCS_SOFT) && !is_soft_discs(MPPI_MODEL_NAV2D_DISCS) &&
              !is_soft_discs(MPPI_MODEL_RACING_DISCS) && has_discs(MPPI_MODEL_NAV2D_DISCS_SOFT) && has_discs(MPPI_MODEL_RACING_DISCS_SOFT)) ? 1 : 0;
}

extern "C" int soft_discs_emul_nav2d(int fast, int kind, float a, float b, const float* params, const uint8_t* cells, int nx, int ny,
                                     float cell, float ox, float oy, const float* table8, int rows, int n, const float* x0,
                                     const float* U, int N, int T, float* costs, float* S_out) {
    if (n < 0 || n > MPPI_MAX_DISCS || rows < T || T < 1 || N < 1 || kind < 0 || kind > 2) return -1;
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    for (int i = 0; i < MPPI_NP_COUNT; ++i) ctx.P[i] = params[i];
    ctx.maps[0] = MapView{cells, nx, ny, cell, 1.0f / cell, ox, oy};
    ctx.ref = table8;
    ctx.ref_rows = rows;
    ctx.u_in_bounds = ctx.wrap_safe = 1;
    const int model = kind == 0 ? MPPI_MODEL_NAV2D_DISCS_SOFT : MPPI_MODEL_NAV2D_DISCS;
    set_disc_count(ctx, model, n);
    if (kind == 0) {
        set_disc_soft(ctx, model, a, b);
        const DiscSoft f = disc_soft(ctx, model);
        if (f.a != a || f.b != b || disc_count(ctx, model) != n) return -2;
    }
    if (kind == 0) walk_level<MPPI_MODEL_NAV2D_DISCS_SOFT, false>(fast, ctx, x0, U, N, T, costs, S_out);
    else if (kind == 1) walk_level<MPPI_MODEL_NAV2D_DISCS, false>(fast, ctx, x0, U, N, T, costs, S_out);
    else walk_level<MPPI_MODEL_NAV2D, false>(fast, ctx, x0, U, N, T, costs, S_out);
    return 0;
}

extern "C" int soft_discs_emul_racing(int fast, int kind, float a, float b, const float* params, const uint8_t* obst,
                                      const uint8_t* lane, int nx, int ny, float cell, float ox, float oy, const float* ref8,
                                      const float* discs8, int rows, int n, const float* x0, const float* U, int N, int T,
                                      float* costs, float* S_out) {
    if (n < 0 || n > MPPI_MAX_DISCS || rows < T || T < 1 || N < 1 || kind < 0 || kind > 2) return -1;
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    for (int i = 0; i < MPPI_RP_COUNT; ++i) ctx.P[i] = params[i];
    ctx.maps[0] = MapView{obst, nx, ny, cell, 1.0f / cell, ox, oy};
    ctx.maps[1] = MapView{lane, nx, ny, cell, 1.0f / cell, ox, oy};
    const int model = kind == 0 ? MPPI_MODEL_RACING_DISCS_SOFT : kind == 1 ? MPPI_MODEL_RACING_DISCS : MPPI_MODEL_RACING;
    const int stride = ref_stride(model), off = disc_offset(model);
    std::vector<float> tab((size_t)rows * stride);  // exactly the rows: the walk must not read past row T-1
    for (int t = 0; t < rows; ++t) {
        std::memcpy(tab.data() + (size_t)t * stride, ref8 + (size_t)t * RACING_REF_ROW, sizeof(float) * RACING_REF_ROW);
        if (kind != 2) std::memcpy(tab.data() + (size_t)t * stride + off, discs8 + (size_t)t * DISC_ROW, sizeof(float) * DISC_ROW);
    }
    ctx.ref = tab.data();
    ctx.ref_rows = rows;
    ctx.tan_small = 1;  // (racing's own flag: the disc count of this model does not ride there)
    if (kind != 2) {
        set_disc_count(ctx, model, n);
        if (disc_count(ctx, model) != n || ctx.tan_small != 1) return -2;
    }
    if (kind == 0) {
        set_disc_soft(ctx, model, a, b);
        const DiscSoft f = disc_soft(ctx, model);
        if (f.a != a || f.b != b || disc_count(ctx, model) != n) return -2;  // (the count and the coefficients are neighbours)
    }
    ctx.inv_L = 1.0f / params[MPPI_RP_L];
    ctx.unit_L = 0;
    ctx.u_in_bounds = ctx.wrap_safe = 1;
    if (kind == 0) walk_level<MPPI_MODEL_RACING_DISCS_SOFT, true>(fast, ctx, x0, U, N, T, costs, S_out);
    else if (kind == 1) walk_level<MPPI_MODEL_RACING_DISCS, true>(fast, ctx, x0, U, N, T, costs, S_out);
    else walk_level<MPPI_MODEL_RACING, true>(fast, ctx, x0, U, N, T, costs, S_out);
    return 0;
}

#ifdef SOFT_DISCS_EMUL_MAIN
static bool read_exact(std::FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 4;
    int32_t hd[9];
    int cases = 0;
    while (read_exact(in, hd, sizeof(hd))) {
        const int racing = hd[0], fast = hd[1], kind = hd[2], N = hd[3], T = hd[4], rows = hd[5], n = hd[6], nx = hd[7], ny = hd[8];
        if (N < 1 || T < 1 || rows < T || nx < 1 || ny < 1) return 5;
        const size_t ds = racing ? 4 : 3;
        std::vector<float> ab(2), params(racing ? (size_t)MPPI_RP_COUNT : (size_t)MPPI_NP_COUNT), geom(3), ref(racing ? (size_t)rows * RACING_REF_ROW : 0),
            discs((size_t)rows * DISC_ROW), x0(ds), U((size_t)N * T * 2), costs((size_t)N);
        std::vector<uint8_t> obst((size_t)nx * ny), lane(racing ? (size_t)nx * ny : 0);
        if (!read_exact(in, ab.data(), 8) || !read_exact(in, params.data(), 4 * params.size()) || !read_exact(in, geom.data(), 12) ||
            !read_exact(in, obst.data(), obst.size()) || !read_exact(in, lane.data(), lane.size()) ||
            !read_exact(in, ref.data(), 4 * ref.size()) || !read_exact(in, discs.data(), 4 * discs.size()) ||
            !read_exact(in, x0.data(), 4 * ds) || !read_exact(in, U.data(), 4 * U.size()))
            return 6;
        const int rc = racing ? soft_discs_emul_racing(fast, kind, ab[0], ab[1], params.data(), obst.data(), lane.data(), nx, ny, geom[0],
                                                       geom[1], geom[2], ref.data(), discs.data(), rows, n, x0.data(), U.data(), N, T,
                                                       costs.data(), nullptr)
                              : soft_discs_emul_nav2d(fast, kind, ab[0], ab[1], params.data(), obst.data(), nx, ny, geom[0], geom[1], geom[2],
                                                      discs.data(), rows, n, x0.data(), U.data(), N, T, costs.data(), nullptr);
        if (rc != 0) return 7;
        std::fwrite(costs.data(), 4, costs.size(), out);
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("soft_discs_emul: %d cases\n", cases);
    return 0;
}
#endif
