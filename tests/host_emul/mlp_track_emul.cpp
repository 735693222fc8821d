// Host build of the learned-dynamics functors' TRACKING cost (MlpModel::cost of mppi_playground_amd/csrc/mppi_models.inc with a
// reference table and an angular mask: include/mppi_hip.h, mppi_set_mlp_reference / mppi_set_mlp_angular) for
// tests/test_mlp_tracking_host.py.  TEST-ONLY: the product never loads this.  Built twice from this one text, as
// tests/host_emul/mlp8_emul.cpp is:
//   as a shared library (ctypes: mlp_track_emul_rollout), and
//   with -DMLP_TRACK_EMUL_MAIN -fsanitize=address,undefined as a stand-alone program: `mlp_track_emul_main cases.bin costs.bin`
//   walks the cases the test wrote (per case: int32 {ds, dc, fast, hidden layers, tanh, residual, N, T, table floats,
//   reference rows, angular mask}, then the table, 2 * ds + dc parameters, x0[ds], U[N][T][dc] and the reference
//   [rows][2 * ds] as float32) into heap buffers of exactly those sizes — the reference has exactly T rows, so a read of row T
//   is a sanitizer report — and writes the costs; without arguments it walks generated batches of every (id, layers,
//   activation, math level) with a reference of exactly T rows and both end components angular.
// The context is the tests' usual one: memset to 0, the parameters, NaN behind them, then the two things this feature adds
// through the accessors of mppi_models.hpp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mppi_playground_amd/csrc/mppi_models.hpp"

using namespace mppi;

template <int MODEL, bool FAST>
static void walk(const float* params, int n_params, const float* table, int flags, const float* ref, uint32_t angular,
                 const float* x0, const float* U, int N, int T, float* costs, float* S_out) {
    using M = ModelT<MODEL, FAST ? 1 : 0>;
    constexpr int DS = M::DS, DC = M::DC;
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    for (int i = 0; i < n_params; ++i) ctx.P[i] = params[i];
    for (int i = n_params; i < MPPI_MAX_PARAMS; ++i) ctx.P[i] = NAN;  // (a read past the parameters shows in the costs)
    ctx.ref = table;
    ctx.ref_rows = mlp_flags_word(flags, angular);
    set_mlp_reference(ctx, ref);
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

// ref may be null (no reference); otherwise [ref_rows][2 * ds] with ref_rows >= T
extern "C" int mlp_track_emul_rollout(int ds, int dc, int fast, const float* table, int n_floats, int hidden_layers, int use_tanh,
                                      int residual, const float* params, int n_params, const float* ref, int ref_rows,
                                      uint32_t angular, const float* x0, const float* U, int N, int T, float* costs, float* S_out) {
    const bool ok4 = ds == 4 && (dc == 1 || dc == 2), ok8 = ds == 8 && (dc == 1 || dc == 2 || dc == 4);
    if ((!ok4 && !ok8) || n_floats != mlp_table_floats(ds, dc) || n_params != 2 * ds + dc || (ref && ref_rows < T) || (angular >> ds))
        return -1;
    const int flags = (hidden_layers == 2 ? MLP_TWO_LAYERS : 0) | (use_tanh ? MLP_TANH : 0) | (residual ? MLP_RESIDUAL : 0);
#define WALK(MODEL)                                                                                                  \
    do {                                                                                                             \
        if (fast) walk<MODEL, true>(params, n_params, table, flags, ref, angular, x0, U, N, T, costs, S_out);        \
        else walk<MODEL, false>(params, n_params, table, flags, ref, angular, x0, U, N, T, costs, S_out);            \
    } while (0)
    if (ds == 4 && dc == 1) WALK(MPPI_MODEL_MLP41);
    else if (ds == 4) WALK(MPPI_MODEL_MLP42);
    else if (dc == 1) WALK(MPPI_MODEL_MLP81);
    else if (dc == 2) WALK(MPPI_MODEL_MLP82);
    else WALK(MPPI_MODEL_MLP84);
#undef WALK
    return 0;
}

// the flags word as the library composes it, and the two constants of the wrap (the test compares them with its own)
extern "C" int mlp_track_emul_flags_word(int arch, uint32_t angular) { return mlp_flags_word(arch, angular); }
extern "C" float mlp_track_emul_two_pi() { return MLP_TWO_PI; }
extern "C" float mlp_track_emul_inv_two_pi() { return MLP_INV_TWO_PI; }

#ifdef MLP_TRACK_EMUL_MAIN
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
    int32_t hd[11];
    int cases = 0;
    while (read_exact(in, hd, sizeof(hd))) {
        const int ds = hd[0], dc = hd[1], N = hd[6], T = hd[7], nf = hd[8], rows = hd[9];
        if ((ds != 4 && ds != 8) || dc < 1 || dc > 4 || N < 1 || T < 1 || nf < 1 || rows < 0) return 5;
        std::vector<float> table((size_t)nf), params((size_t)2 * ds + dc), x0((size_t)ds), U((size_t)N * T * dc), costs((size_t)N);
        std::vector<float> ref((size_t)rows * 2 * ds);  // (exactly `rows` rows on the heap)
        if (!read_exact(in, table.data(), 4 * table.size()) || !read_exact(in, params.data(), 4 * params.size()) ||
            !read_exact(in, x0.data(), 4 * x0.size()) || !read_exact(in, U.data(), 4 * U.size()) ||
            (rows && !read_exact(in, ref.data(), 4 * ref.size())))
            return 6;
        if (mlp_track_emul_rollout(ds, dc, hd[2], table.data(), nf, hd[3], hd[4], hd[5], params.data(), (int)params.size(),
                                   rows ? ref.data() : nullptr, rows, (uint32_t)hd[10], x0.data(), U.data(), N, T, costs.data(),
                                   nullptr) != 0)
            return 7;
        std::fwrite(costs.data(), 4, costs.size(), out);
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("mlp_track_emul: %d cases\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_file(argv[1], argv[2]);
    double sum = 0.0;
    int runs = 0;
    const int ids[5][2] = {{4, 1}, {4, 2}, {8, 1}, {8, 2}, {8, 4}};
    for (const auto& id : ids)
        for (int layers = 1; layers <= 2; ++layers)
            for (int th = 0; th <= 1; ++th)
                for (int fast = 0; fast <= 1; ++fast) {
                    const int ds = id[0], dc = id[1], N = 37, T = 9;
                    std::vector<float> table((size_t)mlp_table_floats(ds, dc));
                    for (float& w : table) w = 0.1f * rnd();
                    std::vector<float> params((size_t)2 * ds + dc);
                    for (float& p : params) p = 0.5f + 0.5f * rnd();
                    std::vector<float> ref((size_t)T * 2 * ds);  // exactly T rows: goals in +-9 (they wrap), weights in [0.5, 1.5)
                    for (int t = 0; t < T; ++t)
                        for (int m = 0; m < ds; ++m) {
                            ref[(size_t)t * 2 * ds + m] = 9.0f * rnd();
                            ref[(size_t)t * 2 * ds + ds + m] = 1.0f + 0.5f * rnd();
                        }
                    std::vector<float> U((size_t)N * T * dc), costs((size_t)N), S((size_t)N * (T + 1) * ds), x0((size_t)ds);
                    for (float& u : U) u = rnd();
                    for (float& x : x0) x = 0.5f * rnd();
                    const uint32_t angular = 1u | (1u << (ds - 1));
                    if (mlp_track_emul_rollout(ds, dc, fast, table.data(), (int)table.size(), layers, th, 1, params.data(),
                                               (int)params.size(), ref.data(), T, angular, x0.data(), U.data(), N, T, costs.data(),
                                               S.data()) != 0)
                        return 2;
                    for (float c : costs) {
                        if (!std::isfinite(c)) return 3;
                        sum += c;
                    }
                    ++runs;
                }
    std::printf("mlp_track_emul: %d runs, checksum %.9g\n", runs, sum);
    return 0;
}
#endif
