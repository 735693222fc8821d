// Host build of the 8-state learned-dynamics functors (Model<MPPI_MODEL_MLP81 / MLP82 / MLP84> of
// mppi_playground_amd/csrc/mppi_models.inc) for tests/test_mlp8_host.py.  TEST-ONLY: the product never loads this.  Built twice
// from this one text, as tests/host_emul/mlp_emul.cpp is for the 4-state ids:
//   as a shared library (ctypes: mlp8_emul_rollout), and
//   with -DMLP8_EMUL_MAIN -fsanitize=address,undefined as a stand-alone program: `mlp8_emul_main cases.bin costs.bin` walks the
//   cases the test wrote (per case: int32 {dc, fast, hidden layers, tanh, residual, N, T, table floats}, then the table,
//   16 + dc parameters, x0[8] and U[N][T][dc] as float32) into heap buffers of exactly those sizes — a read past the table,
//   the parameters or an action row is a sanitizer report — and writes the costs; without arguments it walks generated
//   batches of every (model, layers, activation, residual, math level).
// The trajectory walk is trajectory_cost() of mppi_rollout.hpp on actions the caller has already clamped.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mppi_playground_amd/csrc/mppi_models.hpp"

using namespace mppi;

template <int MODEL, bool FAST>
static void walk(const float* params, int n_params, const float* table, int flags, const float* x0, const float* U, int N, int T,
                 float* costs, float* S_out) {
    using M = ModelT<MODEL, FAST ? 1 : 0>;
    constexpr int DS = M::DS, DC = M::DC;
    static_assert(DS == 8, "the 8-state ids");
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    for (int i = 0; i < n_params; ++i) ctx.P[i] = params[i];
    // (the parameters the functor may read are the caller's exact count: the rest of ctx.P is poisoned with NaN, so a read
    // past them shows in the costs)
    for (int i = n_params; i < MPPI_MAX_PARAMS; ++i) ctx.P[i] = NAN;
    ctx.ref = table;
    ctx.ref_rows = flags;
    for (int i = 0; i < N; ++i) {
        float s[DS], zero[DC], pu[DC];
        bool bad = false;
        for (int j = 0; j < DS; ++j) s[j] = x0[j];
        for (int k = 0; k < DC; ++k) zero[k] = pu[k] = 0.0f;
        CostSum<exact_cost_sum(MODEL)> acc;
        for (int t = 0; t < T; ++t) {
            const float* u = U + ((size_t)i * T + t) * DC;
            float sn[DS], ss[DS];
            M::step(ctx, s, u, sn, ss, bad);
            acc.add(M::cost(ctx, M::load_k(nullptr, t), ss, u, pu, bad));
            for (int j = 0; j < DS; ++j) {
                if (S_out) S_out[((size_t)i * (T + 1) + t) * DS + j] = ss[j];
                s[j] = sn[j];
            }
        }
        for (int j = 0; j < DS; ++j)
            if (S_out) S_out[((size_t)i * (T + 1) + T) * DS + j] = s[j];
        costs[i] = acc.total(M::cost(ctx, M::load_k(nullptr, T - 1), s, zero, pu, bad));
        if (bad) costs[i] = NAN;  // (these models have no validity range: never taken)
    }
}

extern "C" int mlp8_emul_rollout(int dc, int fast, const float* table, int n_floats, int hidden_layers, int use_tanh, int residual,
                                 const float* params, int n_params, const float* x0, const float* U, int N, int T, float* costs,
                                 float* S_out) {
    if ((dc != 1 && dc != 2 && dc != 4) || n_floats != mlp_table_floats(8, dc) || n_params != MPPI_MP8_R + dc) return -1;
    const int flags = (hidden_layers == 2 ? MLP_TWO_LAYERS : 0) | (use_tanh ? MLP_TANH : 0) | (residual ? MLP_RESIDUAL : 0);
#define WALK(MODEL)                                                                                   \
    do {                                                                                              \
        if (fast) walk<MODEL, true>(params, n_params, table, flags, x0, U, N, T, costs, S_out);       \
        else walk<MODEL, false>(params, n_params, table, flags, x0, U, N, T, costs, S_out);           \
    } while (0)
    if (dc == 1) WALK(MPPI_MODEL_MLP81);
    else if (dc == 2) WALK(MPPI_MODEL_MLP82);
    else WALK(MPPI_MODEL_MLP84);
#undef WALK
    return 0;
}

// the sizes and ids as the library's headers state them (the test compares them with its own)
extern "C" int mlp8_emul_table_floats(int dc) { return mlp_table_floats(8, dc); }
extern "C" int mlp8_emul_param_count(int dc) { return dc == 1 ? MPPI_MP8_COUNT81 : dc == 2 ? MPPI_MP8_COUNT82 : dc == 4 ? MPPI_MP8_COUNT84 : -1; }
extern "C" int mlp8_emul_model_id(int dc) { return dc == 1 ? MPPI_MODEL_MLP81 : dc == 2 ? MPPI_MODEL_MLP82 : dc == 4 ? MPPI_MODEL_MLP84 : -1; }

#ifdef MLP8_EMUL_MAIN
// xorshift: deterministic values in [-1, 1)
static uint32_t g_rng = 2463534242u;
static float rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
    return (float)(int32_t)g_rng * (1.0f / 2147483648.0f);
}

static bool read_exact(std::FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

static int run_file(const char* in_path, const char* out_path) {
    std::FILE* in = std::fopen(in_path, "rb");
    std::FILE* out = std::fopen(out_path, "wb");
    if (!in || !out) return 4;
    int32_t hd[8];
    int cases = 0;
    while (read_exact(in, hd, sizeof(hd))) {
        const int dc = hd[0], N = hd[5], T = hd[6], nf = hd[7];
        if ((dc != 1 && dc != 2 && dc != 4) || N < 1 || T < 1 || nf < 1) return 5;
        std::vector<float> table((size_t)nf), params((size_t)16 + dc), x0(8), U((size_t)N * T * dc), costs((size_t)N);
        if (!read_exact(in, table.data(), 4 * table.size()) || !read_exact(in, params.data(), 4 * params.size()) ||
            !read_exact(in, x0.data(), 32) || !read_exact(in, U.data(), 4 * U.size()))
            return 6;
        if (mlp8_emul_rollout(dc, hd[1], table.data(), nf, hd[2], hd[3], hd[4], params.data(), (int)params.size(), x0.data(),
                              U.data(), N, T, costs.data(), nullptr) != 0)
            return 7;
        std::fwrite(costs.data(), 4, costs.size(), out);
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("mlp8_emul: %d cases\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_file(argv[1], argv[2]);
    double sum = 0.0;
    int runs = 0;
    for (int dc = 1; dc <= 4; dc *= 2)
        for (int layers = 1; layers <= 2; ++layers)
            for (int th = 0; th <= 1; ++th)
                for (int res = 0; res <= 1; ++res)
                    for (int fast = 0; fast <= 1; ++fast) {
                        // (heap vectors of the exact sizes: a read past the table or an action row is a sanitizer report)
                        std::vector<float> table((size_t)mlp_table_floats(8, dc));
                        for (float& w : table) w = 0.1f * rnd();
                        std::vector<float> params((size_t)16 + dc);
                        for (float& p : params) p = 0.5f + 0.5f * rnd();
                        const int N = 37, T = 9;
                        std::vector<float> U((size_t)N * T * dc), costs((size_t)N), S((size_t)N * (T + 1) * 8);
                        for (float& u : U) u = rnd();
                        const std::vector<float> x0 = {0.3f, -0.2f, 0.5f, 0.1f, -0.4f, 0.25f, 0.15f, -0.1f};
                        if (mlp8_emul_rollout(dc, fast, table.data(), (int)table.size(), layers, th, res, params.data(),
                                              (int)params.size(), x0.data(), U.data(), N, T, costs.data(), S.data()) != 0)
                            return 2;
                        for (float c : costs) {
                            if (!std::isfinite(c)) return 3;
                            sum += c;
                        }
                        ++runs;
                    }
    std::printf("mlp8_emul: %d runs, checksum %.9g\n", runs, sum);
    return 0;
}
#endif
