// Exhaustive host proof of the two shortened sequences of the FAST racing / nav2d step (mppi_models.inc):
//   1. wrap_inc_f  — every float x in [-2pi, 2pi] (a wrapped heading in [-pi, pi) plus an increment the host bounds
//      below pi, ctx.wrap_safe): the shipped floor-based sequence (mppi_models.inc, its mppi::strict and mppi::fused
//      copies) against the branchy one it replaced, bit for bit;
//   2. map index   — every float p of a position clamp box [lo, hi]: the padded grid's biased index with the origin
//      and the rounding constant folded into one add, fl(q + fl(o + 1.5*2^23)), against fl(fl(q + o) + 1.5*2^23),
//      q = RN(p / cell); also the single FMA fl(p * RN(1/cell) + fl(o + 1.5*2^23)).  Neither is exact on the racing
//      or the nav2d map (the double rounding of the reference at fl(q + o) = n + 1/2 is not reproduced), so the kernels
//      keep the five-instruction index; the counts are the record of why.
// Build with clang++, so that mppi_models.hpp's `#pragma clang fp contract(fast)` holds for the mppi::fused copy as it does
// on the device (g++ ignores the pragma and would compile both copies without contraction); run on the host, at most
// 16 threads:
//   clang++ -O2 -std=c++17 -ffp-contract=off -mfma -pthread -o /tmp/enum_wrap_index scripts/enum/enum_wrap_index.cpp
//   /tmp/enum_wrap_index [threads]
// (wrap_inc_f holds no contractible a * b + c in any case: the FMA is explicit, the product feeds floor and the first sum
// feeds the product.)
// Recorded output: profiles/r07_enum_wrap_index.txt.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../mppi_playground_amd/csrc/mppi_models.hpp"

static const float PI_F = 3.14159274f, TWO_PI_F = 6.28318548f, INV_TWO_PI_F = 0.159154937f, MAGIC = 12582912.0f;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float from(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// the sequence of rounds 1-6
static float wrap_old(float x) {
    const float a = x + PI_F;
    float r = a;
    if (a >= TWO_PI_F) r = a - TWO_PI_F;
    if (r < 0.0f) r += TWO_PI_F;
    return r - PI_F;
}
// the shipped sequence (5 VALU: add, mul, floor, fma, sub), both copies of the model code
static float wrap_new(float x) { return mppi::strict::wrap_inc_f(x); }
static float wrap_new_fused(float x) { return mppi::fused::wrap_inc_f(x); }

// Float p <-> a monotone integer key (so that [lo, hi] is one integer range).
static int64_t key(float f) { const uint32_t u = bits(f); return (u & 0x80000000u) ? -(int64_t)(u & 0x7fffffffu) : (int64_t)u; }
static float unkey(int64_t k) { return k < 0 ? from(0x80000000u | (uint32_t)(-k)) : from((uint32_t)k); }

template <class F>
static void parallel(int64_t k0, int64_t k1, int nt, F f) {  // f(k) over every key in [k0, k1]; -0 is covered as +0's twin
    std::vector<std::thread> th;
    const int64_t n = k1 - k0 + 1;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([=] {
            for (int64_t k = k0 + n * t / nt; k < k0 + n * (t + 1) / nt; ++k) f(k);
        });
    for (auto& x : th) x.join();
}

int main(int argc, char** argv) {
    const int nt = argc > 1 ? std::max(1, std::min(16, atoi(argv[1]))) : 16;
    int fails = 0;
    {   // 1. heading wrap
        std::atomic<uint64_t> bad{0};
        const int64_t k0 = key(-TWO_PI_F), k1 = key(TWO_PI_F);
        parallel(k0, k1, nt, [&](int64_t k) {
            const float x = unkey(k);
            const uint32_t ref = bits(wrap_old(x));
            uint64_t b = (ref != bits(wrap_new(x))) + (ref != bits(wrap_new_fused(x)));
            if (k == 0) b += (bits(wrap_old(-0.0f)) != bits(wrap_new(-0.0f))) + (bits(wrap_old(-0.0f)) != bits(wrap_new_fused(-0.0f)));
            if (b) bad += b;
        });
        const uint64_t total = (uint64_t)(k1 - k0 + 2);  // + the -0 twin
        printf("wrap_inc_f (mppi::strict and mppi::fused): %llu floats x in [-2pi, 2pi]: %llu mismatches (k = floor(fl(x + pi) * %.9g))\n",
               (unsigned long long)total, (unsigned long long)bad.load(), INV_TWO_PI_F);
        fails += bad.load() != 0;
    }
    struct Box { const char* name; float cell, o, lo, hi; };
    const Box boxes[] = {{"racing (80 m map)", 0.1f, 400.0f, -40.0f, 40.0f},
                         {"nav2d (20 m map)", 0.1f, 100.0f, -10.0f, 10.0f}};
    for (const Box& bx : boxes) {  // 2. map index
        const float inv = 1.0f / bx.cell, K = bx.o + MAGIC;
        std::atomic<uint64_t> bad_fold{0}, bad_fma{0};
        const int64_t k0 = key(bx.lo), k1 = key(bx.hi);
        parallel(k0, k1, nt, [&](int64_t k) {
            const float p = unkey(k);
            const float q = p / bx.cell;  // = the device's Markstein quotient (tests/test_model_functors_host.py)
            const uint32_t ref = bits((q + bx.o) + MAGIC);
            if (bits(q + K) != ref) ++bad_fold;
            if (bits(fmaf(p, inv, K)) != ref) ++bad_fma;
        });
        printf("map index, %s: cell %.9g, origin %g, %llu floats p in [%g, %g]: fold %llu mismatches, single fma %llu mismatches\n",
               bx.name, bx.cell, bx.o, (unsigned long long)(k1 - k0 + 1), bx.lo, bx.hi, (unsigned long long)bad_fold.load(),
               (unsigned long long)bad_fma.load());
    }
    return fails;
}
