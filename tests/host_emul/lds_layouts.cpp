// The dynamic-LDS layouts of csrc/mppi_lds.hpp, walked on the host (tests/test_lds_layouts_host.py): `lds_layouts <layout>`
// writes one record of int64 per case to stdout: the case's parameters, floats(), then {offset, size} of every region in
// the order the kernel lays them out.  The region SIZES are stated here, from what each kernel writes to the region; the
// offsets and the total come from the header.  `lds_layouts all` walks every layout (the sanitizer build runs that).
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../mppi_playground_amd/csrc/mppi_lds.hpp"

using namespace mppi;
using i64 = long long;

static std::vector<i64> g_out;
static void emit(std::initializer_list<i64> v) { g_out.insert(g_out.end(), v); }

static std::vector<int> horizons() {
    std::vector<int> t;
    for (int i = 1; i <= 70; ++i) t.push_back(i);
    t.push_back(255);
    t.push_back(1000);
    return t;
}
// 0 (no filter), then every window mppi_set_sg_filter admits at this horizon: odd, <= 255, window / 2 <= 2T - 1
static std::vector<int> windows(int T) {
    std::vector<int> w{0};
    for (int k = 3; k <= 255 && k / 2 <= 2 * T - 1; k += 2) w.push_back(k);
    return w;
}
static int groups(int row) { return (row + 3) / 4; }

static void rollout() {
    for (int T : horizons()) for (int dc : {1, 2, 4}) for (int krow : {0, 8}) for (int ac : {0, 1}) {
        const int row = T * dc, R = groups(row);
        emit({T, dc, krow, ac, R, row, (i64)RolloutLds::floats(R, T, row, krow, ac != 0),
              RolloutLds::mean(), 4 * R, RolloutLds::zeros(R), 4 * R, RolloutLds::g(R), ac ? 4 * R : 0,
              RolloutLds::ktab(R, ac != 0), T * krow,
              RolloutLds::rider_act(), row, RolloutLds::rider_x0(row), MPPI_MAX_DIM_STATE});
    }
}
static void fused() {
    for (int T : horizons()) for (int dc : {1, 2, 4}) for (int krow : {0, 8}) for (int w : windows(T)) {
        const int row = T * dc, R = groups(row);
        emit({T, dc, krow, w, R, row, (i64)FusedLds::floats(R, T, row, dc, krow, w),
              FusedLds::mean(), 4 * R, FusedLds::zeros(R), 4 * R, FusedLds::ktab(R), T * krow,
              FusedLds::act(R, T, krow), row, FusedLds::sum(R, T, row, krow), MPPI_SUMMARY_HEAD + row,
              FusedLds::yp(R, T, row, krow), w ? (2 * T - 1 + 2 * (w / 2)) * dc : 0});
    }
}
static void finalize() {
    for (int T : horizons()) for (int dc : {1, 2, 3, 4, 8, 64}) for (int world : {1, 2, 3, 8}) for (int fold : {0, 1})
        for (int w : windows(T)) {
            const int row = T * dc;
            emit({T, dc, world, fold, w, row, (i64)FinalizeLds::floats(T, row, dc, world, w, fold != 0),
                  FinalizeLds::act(), row, FinalizeLds::sum(row), (i64)world * (MPPI_SUMMARY_HEAD + row),
                  FinalizeLds::yp(row, world), w ? (2 * T - 1 + 2 * (w / 2)) * dc : 0,
                  FinalizeLds::fold(T, row, dc, world, w), fold ? 64 * (row + 3) : 0});
        }
}
static void state_seq() {
    for (int T : horizons()) for (int dc : {1, 2, 4}) {
        const int row = T * dc;
        emit({T, dc, row, (i64)StateSeqLds::floats(row), StateSeqLds::act(), row, StateSeqLds::x0(row), MPPI_MAX_DIM_STATE});
    }
}
static void wave() {
    for (int T : horizons()) for (int dc : {1, 2, 4}) for (int ds : {2, 3, 4, 7}) {
        const int row = T * dc, R = groups(row), pw = WaveRolloutLds::per_wave(R, T, ds);
        std::vector<i64> rec{T, dc, ds, R, (i64)WaveRolloutLds::floats(R, T, ds)};
        for (int wv = 0; wv < 4; ++wv)
            rec.insert(rec.end(), {(i64)wv * pw + WaveRolloutLds::u(), 4 * R, (i64)wv * pw + WaveRolloutLds::s(R), (i64)(T + 1) * ds});
        g_out.insert(g_out.end(), rec.begin(), rec.end());
    }
}
static void topk() {
    for (int T : horizons()) for (int dc : {1, 2, 4}) for (int sorted : {0, 1}) for (int gen : {0, 1}) {
        const int row = T * dc, R = groups(row);
        const bool pregen = !sorted && gen && R <= 32;
        emit({T, dc, sorted, gen, R, (i64)TopkLds::floats(R, sorted != 0, gen != 0), TopkLds::mean(), 4 * R, TopkLds::zeros(R), 4 * R,
              TopkLds::noise(R), pregen ? 4 * 64 * R : 0});
        if (pregen != TopkLds::pregen(R, sorted != 0, gen != 0)) { std::fprintf(stderr, "pregen(%d, %d, %d)\n", R, sorted, gen); std::exit(1); }
    }
}
static void brent() {
    for (int per_thread = 1; per_thread <= 33; ++per_thread) for (int threads : {256, 512, 768, 1024})
        emit({per_thread, threads, (i64)BrentStageLds::floats(per_thread, threads), BrentStageLds::cost(), (i64)per_thread * threads});
}

int main(int argc, char** argv) {
    struct { const char* name; void (*fn)(); } layouts[] = {{"rollout", rollout}, {"fused", fused}, {"finalize", finalize},
        {"state_seq", state_seq}, {"wave", wave}, {"topk", topk}, {"brent", brent}};
    const char* which = argc > 1 ? argv[1] : "all";
    bool any = false;
    for (auto& l : layouts)
        if (!std::strcmp(which, "all") || !std::strcmp(which, l.name)) { l.fn(); any = true; }
    if (!any) { std::fprintf(stderr, "unknown layout %s\n", which); return 2; }
    return std::fwrite(g_out.data(), sizeof(i64), g_out.size(), stdout) == g_out.size() ? 0 : 1;
}
