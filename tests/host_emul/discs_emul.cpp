// Host build of the moving-disc functor (Model<MPPI_MODEL_NAV2D_DISCS> of mppi_playground_amd/csrc/mppi_models.inc and
// csrc/mppi_discs.hpp) for tests/test_moving_discs_host.py.  TEST-ONLY: the product never loads this.  Built twice from this
// one text:
//   as a shared library (ctypes: discs_emul_rollout, discs_emul_krow), and
//   with -DDISCS_EMUL_MAIN -fsanitize=address,undefined as a stand-alone program: `discs_emul_main cases.bin costs.bin` walks
//   the cases the test wrote (per case: int32 {fast, plain nav2d, N, T, rows, n, nx, ny}, then 12 parameters, {cell, ox, oy},
//   the nx * ny map bytes, the PADDED table [rows][8][4], x0[3] and U[N][T][2] as float32) in heap buffers of exactly those
//   sizes — a read past a table row or an action row is a sanitizer report — and writes the costs.
// The trajectory walk is trajectory_cost() of mppi_rollout.hpp on actions the caller has already clamped: the stage cost of
// step t reads row t, the terminal cost row T-1.  Level 1 uses the bounds-tested map lookup (`general`): the padded grid is
// a device-side layout of the same cells.
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
        float s[DS], zero[DC], pu[DC];
        bool bad = false;
        for (int j = 0; j < DS; ++j) s[j] = x0[j];
        if (FAST) M::enter_any(s);
        for (int k = 0; k < DC; ++k) zero[k] = pu[k] = 0.0f;
        CostSum<exact_cost_sum(MODEL)> acc;
        for (int t = 0; t < T; ++t) {
            const float* u = U + ((size_t)i * T + t) * DC;
            float sn[DS], ss[DS];
            M::step(ctx, s, u, sn, ss, bad, false, FAST);
            acc.add(M::cost(ctx, M::load_k(ctx.ref, t), ss, u, pu, bad, true));
            for (int j = 0; j < DS; ++j) {
                if (S_out) S_out[((size_t)i * (T + 1) + t) * DS + j] = ss[j];
                s[j] = sn[j];
            }
        }
        for (int j = 0; j < DS; ++j)
            if (S_out) S_out[((size_t)i * (T + 1) + T) * DS + j] = s[j];
        costs[i] = acc.total(M::cost(ctx, M::load_k(ctx.ref, T - 1), s, zero, pu, bad, true));
        if (bad) costs[i] = NAN;  // (never taken: the entry is general)
    }
}

extern "C" int discs_emul_krow() { return ModelT<MPPI_MODEL_NAV2D_DISCS, 0>::KROW; }

// plain != 0: the plain nav2d functor on the same inputs (the table is not read)
extern "C" int discs_emul_rollout(int fast, int plain, const float* params, const uint8_t* cells, int nx, int ny, float cell,
                                  float ox, float oy, const float* table8, int rows, int n, const float* x0, const float* U,
                                  int N, int T, float* costs, float* S_out) {
    if (n < 0 || n > MPPI_MAX_DISCS || rows < T || T < 1 || N < 1) return -1;
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    for (int i = 0; i < MPPI_NP_COUNT; ++i) ctx.P[i] = params[i];
    ctx.maps[0] = MapView{cells, nx, ny, cell, 1.0f / cell, ox, oy};
    ctx.ref = table8;
    ctx.ref_rows = rows;
    ctx.tan_small = n;  // (disc_count)
    ctx.u_in_bounds = ctx.wrap_safe = 1;
    if (plain) {
        if (fast) walk<MPPI_MODEL_NAV2D, true>(ctx, x0, U, N, T, costs, S_out);
        else walk<MPPI_MODEL_NAV2D, false>(ctx, x0, U, N, T, costs, S_out);
    } else {
        if (fast) walk<MPPI_MODEL_NAV2D_DISCS, true>(ctx, x0, U, N, T, costs, S_out);
        else walk<MPPI_MODEL_NAV2D_DISCS, false>(ctx, x0, U, N, T, costs, S_out);
    }
    return 0;
}

#ifdef DISCS_EMUL_MAIN
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
        std::vector<float> params(MPPI_NP_COUNT), geom(3), table((size_t)rows * 4 * MPPI_MAX_DISCS), x0(3), U((size_t)N * T * 2),
            costs((size_t)N);
        std::vector<uint8_t> cells((size_t)nx * ny);
        if (!read_exact(in, params.data(), 4 * params.size()) || !read_exact(in, geom.data(), 12) ||
            !read_exact(in, cells.data(), cells.size()) || !read_exact(in, table.data(), 4 * table.size()) ||
            !read_exact(in, x0.data(), 12) || !read_exact(in, U.data(), 4 * U.size()))
            return 6;
        if (discs_emul_rollout(fast, plain, params.data(), cells.data(), nx, ny, geom[0], geom[1], geom[2], table.data(), rows, n,
                               x0.data(), U.data(), N, T, costs.data(), nullptr) != 0)
            return 7;
        std::fwrite(costs.data(), 4, costs.size(), out);
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("discs_emul: %d cases\n", cases);
    return 0;
}
#endif
