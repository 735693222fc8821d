// Host build of the learned-dynamics functors' TERMINAL VALUE (MlpModel::value / terminal_with_value of
// mppi_playground_amd/csrc/mppi_models.inc: include/mppi_hip.h, mppi_set_mlp_value) for tests/test_mlp_value_host.py.
// TEST-ONLY: the product never loads this.  Built as a shared library (ctypes) and, with -DMLP_VALUE_EMUL_MAIN
// -fsanitize=address,undefined, as a stand-alone program that walks generated batches of every (id, value depth, activation,
// math level, replace flag) with a value table of exactly mlp_value_floats(ds) heap floats.
// The context is the tests' usual one: memset to 0, the parameters, NaN behind them, then what the features add through the
// accessors of mppi_models.hpp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mppi_playground_amd/csrc/mppi_models.hpp"

using namespace mppi;

template <int MODEL, bool FAST>
static void walk(const float* params, int n_params, const float* table, int flags, const float* ref, uint32_t angular,
                 const float* vtable, int vflags, float weight, const float* x0, const float* U, int N, int T, float* costs,
                 float* V_out) {
    using M = ModelT<MODEL, FAST ? 1 : 0>;
    constexpr int DS = M::DS, DC = M::DC;
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    for (int i = 0; i < n_params; ++i) ctx.P[i] = params[i];
    for (int i = n_params; i < MPPI_MAX_PARAMS; ++i) ctx.P[i] = NAN;  // (a read past the parameters shows in the costs)
    ctx.ref = table;
    ctx.ref_rows = mlp_flags_word(flags, angular, vtable ? vflags : 0);
    set_mlp_reference(ctx, ref);
    set_mlp_value(ctx, vtable, weight);
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
            for (int j = 0; j < DS; ++j) s[j] = sn[j];
        }
        float term = M::cost(ctx, M::load_k(nullptr, T - 1), s, zero, pu, bad);
        if (mlp_value_on(ctx)) {  // (the terminal site of trajectory_cost)
            term = M::terminal_with_value(ctx, term, s);
            if (V_out) V_out[i] = M::value(ctx, s);
        }
        costs[i] = acc.total(term);
        if (bad) costs[i] = NAN;  // (these models have no validity range: never taken)
    }
}

// ref may be null (no reference), vtable may be null (no value)
extern "C" int mlp_value_emul_rollout(int ds, int dc, int fast, const float* table, int n_floats, int hidden_layers, int use_tanh,
                                      int residual, const float* params, int n_params, const float* ref, int ref_rows,
                                      uint32_t angular, const float* vtable, int v_floats, int v_layers, int v_tanh, float weight,
                                      int replace_terminal, const float* x0, const float* U, int N, int T, float* costs,
                                      float* V_out) {
    const bool ok4 = ds == 4 && (dc == 1 || dc == 2), ok8 = ds == 8 && (dc == 1 || dc == 2 || dc == 4);
    if ((!ok4 && !ok8) || n_floats != mlp_table_floats(ds, dc) || n_params != 2 * ds + dc || (ref && ref_rows < T) || (angular >> ds) ||
        (vtable && v_floats != mlp_value_floats(ds)))
        return -1;
    const int flags = (hidden_layers == 2 ? MLP_TWO_LAYERS : 0) | (use_tanh ? MLP_TANH : 0) | (residual ? MLP_RESIDUAL : 0);
    const int vflags = (v_layers == 2 ? MLP_VALUE_TWO_LAYERS : 0) | (v_tanh ? MLP_VALUE_TANH : 0) | (replace_terminal ? MLP_VALUE_REPLACE : 0);
#define WALK(MODEL)                                                                                                             \
    do {                                                                                                                        \
        if (fast) walk<MODEL, true>(params, n_params, table, flags, ref, angular, vtable, vflags, weight, x0, U, N, T, costs, V_out); \
        else walk<MODEL, false>(params, n_params, table, flags, ref, angular, vtable, vflags, weight, x0, U, N, T, costs, V_out);    \
    } while (0)
    if (ds == 4 && dc == 1) WALK(MPPI_MODEL_MLP41);
    else if (ds == 4) WALK(MPPI_MODEL_MLP42);
    else if (dc == 1) WALK(MPPI_MODEL_MLP81);
    else if (dc == 2) WALK(MPPI_MODEL_MLP82);
    else WALK(MPPI_MODEL_MLP84);
#undef WALK
    return 0;
}

// what the host composes and sizes, for the test to compare with its own
extern "C" int mlp_value_emul_flags_word(int arch, uint32_t angular, int value) { return mlp_flags_word(arch, angular, value); }
extern "C" int mlp_value_emul_floats(int ds) { return mlp_value_floats(ds); }
extern "C" int mlp_value_emul_tracking(int arch, uint32_t angular, int has_value) {
    static const float one = 1.0f;
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    ctx.ref_rows = mlp_flags_word(arch, angular, 0);
    set_mlp_value(ctx, has_value ? &one : nullptr, 1.0f);
    return mlp_tracking(ctx) ? 1 : 0;
}

#ifdef MLP_VALUE_EMUL_MAIN
// xorshift: deterministic values in [-1, 1)
static uint32_t g_rng = 2463534242u;
static float rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
    return (float)(int32_t)g_rng * (1.0f / 2147483648.0f);
}

int main() {
    double sum = 0.0;
    int runs = 0;
    const int ids[5][2] = {{4, 1}, {4, 2}, {8, 1}, {8, 2}, {8, 4}};
    for (const auto& id : ids)
        for (int vl = 1; vl <= 2; ++vl)
            for (int th = 0; th <= 1; ++th)
                for (int fast = 0; fast <= 1; ++fast)
                    for (int rep = 0; rep <= 1; ++rep) {
                        const int ds = id[0], dc = id[1], N = 23, T = 5;
                        std::vector<float> table((size_t)mlp_table_floats(ds, dc)), vtable((size_t)mlp_value_floats(ds));
                        for (float& w : table) w = 0.1f * rnd();
                        for (float& w : vtable) w = 0.5f * rnd();
                        std::vector<float> params((size_t)2 * ds + dc);
                        for (float& p : params) p = 0.5f + 0.5f * rnd();
                        std::vector<float> U((size_t)N * T * dc), costs((size_t)N), V((size_t)N), x0((size_t)ds);
                        for (float& u : U) u = rnd();
                        for (float& x : x0) x = 0.5f * rnd();
                        if (mlp_value_emul_rollout(ds, dc, fast, table.data(), (int)table.size(), 2, 1, 1, params.data(),
                                                   (int)params.size(), nullptr, 0, 0u, vtable.data(), (int)vtable.size(), vl, th,
                                                   0.75f, rep, x0.data(), U.data(), N, T, costs.data(), V.data()) != 0)
                            return 2;
                        for (float c : costs) {
                            if (!std::isfinite(c)) return 3;
                            sum += c;
                        }
                        ++runs;
                    }
    std::printf("mlp_value_emul: %d runs, checksum %.9g\n", runs, sum);
    return 0;
}
#endif
