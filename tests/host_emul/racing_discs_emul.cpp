// Host build of the racing-among-discs functor (Model<MPPI_MODEL_RACING_DISCS> of mppi_playground_amd/csrc/mppi_models.inc
// and csrc/mppi_discs.hpp) for tests/test_racing_discs_host.py.  TEST-ONLY: the product never loads this.  Built twice from
// this one text:
//   as a shared library (ctypes: racing_discs_emul_rollout, racing_discs_emul_layout), and
//   with -DRACING_DISCS_EMUL_MAIN -fsanitize=address,undefined as a stand-alone program: `racing_discs_emul_main cases.bin
//   costs.bin` walks the cases the test wrote (per case: int32 {fast, plain racing, N, T, rows, n, nx, ny}, then 17 parameters,
//   {cell, ox, oy}, the two nx * ny maps, the reference rows [rows][8], the PADDED discs [rows][8][4], x0[4] and U[N][T][2] as
//   float32) in heap buffers of exactly those sizes — a read past a table row or an action row is a sanitizer report — and
//   writes the costs.
// The step table is built here the way the handle lays it out: [rows][KROW], the reference row in floats 0-7, the discs from
// disc_offset on (plain racing: [rows][8]).  The trajectory walk is trajectory_cost() of mppi_rollout.hpp on actions the
// caller has already clamped: info["prev_action"] of step 0 is U[0] itself, the stage cost of step t reads row t, the
// terminal cost a zero action, the stale U[max(T-2, 0)] and row T-1.  Level 1 uses the bounds-tested map lookups
// (`general`): the padded grid is a device-side layout of the same cells.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mppi_playground_amd/csrc/mppi_models.hpp"

using namespace mppi;

template <int MODEL, bool FAST>
static void walk(const ModelCtx& ctx, const float* x0, const float* U, int N, int T, float* costs, float* S_out) {
    using M = ModelT<MODEL, FAST ? 1 : 0>;
    constexpr int DS = M::DS, DC = M::DC;
    for (int i = 0; i < N; ++i) {
        const float* Ui = U + (size_t)i * T * DC;
        float s[DS], zero[DC], pu[DC], pl[DC];
        bool bad = false;
        for (int j = 0; j < DS; ++j) s[j] = x0[j];
        if (FAST) M::enter_any(s);
        for (int k = 0; k < DC; ++k) { zero[k] = 0.0f; pu[k] = pl[k] = Ui[k]; }
        CostSum<exact_cost_sum(MODEL)> acc;
        for (int t = 0; t < T; ++t) {
            const float* u = Ui + (size_t)t * DC;
            float sn[DS], ss[DS];
            M::step(ctx, s, u, sn, ss, bad, false, FAST, false);
            acc.add(M::cost(ctx, M::load_k(ctx.ref, t), ss, u, pu, bad, true));
            for (int k = 0; k < DC; ++k) { pl[k] = pu[k]; pu[k] = u[k]; }
            for (int j = 0; j < DS; ++j) {
                if (S_out) S_out[((size_t)i * (T + 1) + t) * DS + j] = (t == 0 ? x0[j] : ss[j]);
                s[j] = sn[j];
            }
        }
        for (int j = 0; j < DS; ++j)
            if (S_out) S_out[((size_t)i * (T + 1) + T) * DS + j] = s[j];
        costs[i] = acc.total(M::cost(ctx, M::load_k(ctx.ref, T - 1), s, zero, pl, bad, true));
        if (bad) costs[i] = NAN;  // (never taken: the entry is general)
    }
}

// {KROW, floats of the reference row, first float of the discs, distance in floats from the table's base to the address
//  load_k(tab, t).discs reports for t = 3, sequential cost sum (1) or the double accumulator (0)}
extern "C" void racing_discs_emul_layout(int* out) {
    using M = ModelT<MPPI_MODEL_RACING_DISCS, 0>;
    static float tab[4 * RACING_DISCS_KROW];
    out[0] = M::KROW;
    out[1] = RACING_REF_ROW;
    out[2] = disc_offset(MPPI_MODEL_RACING_DISCS);
    out[3] = (int)(M::load_k(tab, 3).discs - tab);
    out[4] = exact_cost_sum(MPPI_MODEL_RACING_DISCS) ? 0 : 1;
    out[5] = ref_stride(MPPI_MODEL_RACING_DISCS);
    out[6] = ref_stride(MPPI_MODEL_RACING);
    out[7] = RACING_DISCS_SLOT;
}

// plain != 0: the plain racing functor on the same inputs (the discs are not read)
extern "C" int racing_discs_emul_rollout(int fast, int plain, const float* params, const uint8_t* obst, const uint8_t* lane, int nx,
                                         int ny, float cell, float ox, float oy, const float* ref8, const float* discs8, int rows,
                                         int n, const float* x0, const float* U, int N, int T, float* costs, float* S_out) {
    if (n < 0 || n > MPPI_MAX_DISCS || rows < T || T < 1 || N < 1) return -1;
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    for (int i = 0; i < MPPI_RP_COUNT; ++i) ctx.P[i] = params[i];
    ctx.maps[0] = MapView{obst, nx, ny, cell, 1.0f / cell, ox, oy};
    ctx.maps[1] = MapView{lane, nx, ny, cell, 1.0f / cell, ox, oy};
    const int model = plain ? MPPI_MODEL_RACING : MPPI_MODEL_RACING_DISCS;
    const int stride = ref_stride(model), off = disc_offset(MPPI_MODEL_RACING_DISCS);
    std::vector<float> tab((size_t)rows * stride);  // exactly the rows: the walk must not read past row T-1
    for (int t = 0; t < rows; ++t) {
        std::memcpy(tab.data() + (size_t)t * stride, ref8 + (size_t)t * RACING_REF_ROW, sizeof(float) * RACING_REF_ROW);
        if (!plain) std::memcpy(tab.data() + (size_t)t * stride + off, discs8 + (size_t)t * DISC_ROW, sizeof(float) * DISC_ROW);
    }
    ctx.ref = tab.data();
    ctx.ref_rows = rows;
    ctx.tan_small = 1;  // (racing's own flag: the disc count of this model does not ride there)
    if (!plain) {
        set_disc_count(ctx, model, n);
        if (disc_count(ctx, model) != n || ctx.tan_small != 1) return -2;
    }
    ctx.inv_L = 1.0f / params[MPPI_RP_L];
    ctx.unit_L = 0;
    ctx.u_in_bounds = ctx.wrap_safe = 1;
    if (plain) {
        if (fast) walk<MPPI_MODEL_RACING, true>(ctx, x0, U, N, T, costs, S_out);
        else walk<MPPI_MODEL_RACING, false>(ctx, x0, U, N, T, costs, S_out);
    } else {
        if (fast) walk<MPPI_MODEL_RACING_DISCS, true>(ctx, x0, U, N, T, costs, S_out);
        else walk<MPPI_MODEL_RACING_DISCS, false>(ctx, x0, U, N, T, costs, S_out);
    }
    return 0;
}

#ifdef RACING_DISCS_EMUL_MAIN
static bool read_exact(std::FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 4;
    int32_t hd[8];
    int cases = 0;
    while (read_exact(in, hd, sizeof(hd))) {
        const int fast = hd[0], plain = hd[1], N = hd[2], T = hd[3], rows = hd[4], n = hd[5], nx = hd[6], ny = hd[7];
        if (N < 1 || T < 1 || rows < T || nx < 1 || ny < 1) return 5;
        std::vector<float> params(MPPI_RP_COUNT), geom(3), ref((size_t)rows * RACING_REF_ROW), discs((size_t)rows * DISC_ROW), x0(4),
            U((size_t)N * T * 2), costs((size_t)N);
        std::vector<uint8_t> obst((size_t)nx * ny), lane((size_t)nx * ny);
        if (!read_exact(in, params.data(), 4 * params.size()) || !read_exact(in, geom.data(), 12) ||
            !read_exact(in, obst.data(), obst.size()) || !read_exact(in, lane.data(), lane.size()) ||
            !read_exact(in, ref.data(), 4 * ref.size()) || !read_exact(in, discs.data(), 4 * discs.size()) ||
            !read_exact(in, x0.data(), 16) || !read_exact(in, U.data(), 4 * U.size()))
            return 6;
        if (racing_discs_emul_rollout(fast, plain, params.data(), obst.data(), lane.data(), nx, ny, geom[0], geom[1], geom[2],
                                      ref.data(), discs.data(), rows, n, x0.data(), U.data(), N, T, costs.data(), nullptr) != 0)
            return 7;
        std::fwrite(costs.data(), 4, costs.size(), out);
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("racing_discs_emul: %d cases\n", cases);
    return 0;
}
#endif
