// noise_domain — the device values of the noise source (csrc/philox.hpp) over its whole domain, for
// tests/test_gpu_noise_domain.py to compare with float64 (tests/noise_ref.py).  The program only PRODUCES device values (raw
// float32 / uint32 files under the directory it is given) and compares device values with each other; it holds no reference
// arithmetic but the published Philox4x32-10 known answers.
//
//   noise_domain kat DIR       the three Random123 known-answer vectors through both overloads of philox4x32_10 (24 words,
//                              printed and written to kat.u32), and both overloads against each other on 2^20 hashed inputs
//   noise_domain radius DIR    bm_radius(bm_u1_fma(a)) for every a >> 8 -> radius.f32 [2^24]; bm_radius(bm_u1_mul(a)) must be
//                              the same bits
//   noise_domain trig DIR      bm_trig(bm_angle(b)) for every b >> 9 -> cos.f32, sin.f32 [2^23]
//   noise_domain product DIR   box_muller<true> and box_muller<false> on (a, b) against radius[a >> 8] * cos[b >> 9] and
//                              radius[a >> 8] * sin[b >> 9] READ BACK from the two tables (so the tables the test measures
//                              are the factors box_muller multiplies): the four corner pairs and 2^24 hashed pairs
//   noise_domain stream DIR SEED SOLVE FIRST N R
//                              the normals of philox4x32_10((uint32)gi, gi >> 32, r, SOLVE, seed lo, seed hi), gi = FIRST + i,
//                              through box_muller -> stream.f32 [N][4R]
//
// One summary line per mode; exit status 0, 1 on a mismatch between device values (or with the known answers), 2 on a HIP or
// file error or bad arguments.
// Build (the test does it): hipcc + the library's own flags without -shared / -fPIC, -I mppi_playground_amd/csrc.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdint.h>
#include <string>
#include <vector>
#include "philox.hpp"

static constexpr uint32_t N_RADIUS = 1u << 24, N_ANGLE = 1u << 23, N_OVERLOAD = 1u << 20, N_HASHED = 1u << 24;

// {c0, c1, c2, c3, k0, k1} -> {x, y, z, w}: Random123's kat_vectors for philox4x32 with 10 rounds
static const uint32_t KAT_IN[3][6] = {{0u, 0u, 0u, 0u, 0u, 0u},
                                      {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                      {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
static const uint32_t KAT_OUT[3][4] = {{0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
                                       {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
                                       {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};

__host__ __device__ inline uint32_t mix(uint32_t x) {  // (the 32-bit finalizer of MurmurHash3: a fixed integer hash)
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}

// in: [3][6], out: [3][2][4] — vector v through the six-argument overload, then through the nine-argument one
__global__ void kat_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const uint32_t v = threadIdx.x;
    if (v >= 3) return;
    const uint32_t* c = in + 6 * v;
    const mppi::u32x4 six = mppi::philox4x32_10(c[0], c[1], c[2], c[3], c[4], c[5]);
    const mppi::u32x4 nine = mppi::philox4x32_10(c[0], c[1], c[2], c[3], c[4], c[5], c[4], c[5], c[4] + 0x9E3779B9u);
    uint32_t* o = out + 8 * v;
    o[0] = six.x; o[1] = six.y; o[2] = six.z; o[3] = six.w;
    o[4] = nine.x; o[5] = nine.y; o[6] = nine.z; o[7] = nine.w;
}

__global__ __launch_bounds__(256) void overload_kernel(unsigned long long* bad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // the grid covers N_OVERLOAD exactly
    uint32_t w[6];
    for (uint32_t j = 0; j < 6; ++j) w[j] = mix(6u * i + j);
    const mppi::u32x4 six = mppi::philox4x32_10(w[0], w[1], w[2], w[3], w[4], w[5]);
    const mppi::u32x4 nine = mppi::philox4x32_10(w[0], w[1], w[2], w[3], w[4], w[5], w[4], w[5], w[4] + 0x9E3779B9u);
    if (six.x != nine.x || six.y != nine.y || six.z != nine.z || six.w != nine.w) atomicAdd(bad, 1ull);
}

__global__ __launch_bounds__(256) void radius_kernel(float* __restrict__ radius, unsigned long long* bad) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;  // a >> 8: the grid covers 2^24 exactly
    const uint32_t a = n << 8;
    const float r = mppi::bm_radius(mppi::bm_u1_fma(a));
    radius[n] = r;
    if (__float_as_uint(r) != __float_as_uint(mppi::bm_radius(mppi::bm_u1_mul(a)))) atomicAdd(bad, 1ull);
}

__global__ __launch_bounds__(256) void trig_kernel(float* __restrict__ cs, float* __restrict__ sn) {
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;  // b >> 9: the grid covers 2^23 exactly
    float c, s;
    mppi::bm_trig(mppi::bm_angle(m << 9), c, s);
    cs[m] = c;
    sn[m] = s;
}

// pair i < 4: the corners of the two grids; pair 4 + j: hashed words
__global__ __launch_bounds__(256) void product_kernel(const float* __restrict__ radius, const float* __restrict__ cs,
                                                      const float* __restrict__ sn, uint32_t pairs, unsigned long long* bad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pairs) return;
    uint32_t a, b;
    if (i < 4) {
        a = (i & 1u) ? 0xffffffffu : 0u;
        b = (i & 2u) ? 0xffffffffu : 0u;
    } else {
        a = mix(2u * (i - 4u));
        b = mix(2u * (i - 4u) + 1u);
    }
    const float r = radius[a >> 8], c = cs[b >> 9], s = sn[b >> 9];  // indices < 2^24 and < 2^23: inside the tables
    const float want0 = r * c, want1 = r * s;
    float f0, f1, m0, m1;
    mppi::box_muller<true>(a, b, f0, f1);
    mppi::box_muller<false>(a, b, m0, m1);
    const unsigned miss = (__float_as_uint(f0) != __float_as_uint(want0)) + (__float_as_uint(f1) != __float_as_uint(want1)) +
                          (__float_as_uint(m0) != __float_as_uint(want0)) + (__float_as_uint(m1) != __float_as_uint(want1));
    if (miss) atomicAdd(bad, (unsigned long long)miss);
}

__global__ __launch_bounds__(256) void stream_kernel(float* __restrict__ out, uint64_t first, uint32_t n, uint32_t R,
                                                     uint32_t solve, uint32_t seed_lo, uint32_t seed_hi) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)n * R) return;
    const uint32_t i = (uint32_t)(idx / R), r = (uint32_t)(idx - (uint64_t)i * R);
    const uint64_t gi = first + i;
    const mppi::u32x4 x = mppi::philox4x32_10((uint32_t)gi, (uint32_t)(gi >> 32), r, solve, seed_lo, seed_hi);
    float z[4];
    mppi::box_muller(x.x, x.y, z[0], z[1]);
    mppi::box_muller(x.z, x.w, z[2], z[3]);
    for (int j = 0; j < 4; ++j) out[idx * 4 + j] = z[j];
}

#define TRY(x)                                                                                \
    do {                                                                                      \
        const hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) { std::printf("noise_domain: %s: %s\n", #x, hipGetErrorString(e_)); return 2; } \
    } while (0)

static int write_file(const std::string& dir, const char* name, const void* data, size_t bytes) {
    const std::string path = dir + "/" + name;
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::printf("noise_domain: cannot open %s\n", path.c_str()); return 2; }
    const size_t put = std::fwrite(data, 1, bytes, f);
    if (std::fclose(f) != 0 || put != bytes) { std::printf("noise_domain: short write to %s\n", path.c_str()); return 2; }
    return 0;
}

// device floats -> DIR/name
static int save(const std::string& dir, const char* name, const float* dev, size_t count) {
    std::vector<float> host(count);
    TRY(hipMemcpy(host.data(), dev, count * sizeof(float), hipMemcpyDeviceToHost));
    return write_file(dir, name, host.data(), count * sizeof(float));
}

static int fill_tables(float* radius, float* cs, float* sn, unsigned long long* bad) {
    radius_kernel<<<N_RADIUS / 256, 256>>>(radius, bad);
    TRY(hipGetLastError());
    trig_kernel<<<N_ANGLE / 256, 256>>>(cs, sn);
    TRY(hipGetLastError());
    TRY(hipDeviceSynchronize());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: noise_domain kat|radius|trig|product|stream DIR [SEED SOLVE FIRST N R]\n"); return 2; }
    const std::string mode = argv[1], dir = argv[2];
    unsigned long long* bad = nullptr;
    unsigned long long miss = ~0ull;
    TRY(hipMalloc(&bad, 8));
    TRY(hipMemset(bad, 0, 8));

    if (mode == "kat") {
        uint32_t *in = nullptr, *out = nullptr, words[24];
        TRY(hipMalloc(&in, sizeof(KAT_IN)));
        TRY(hipMalloc(&out, sizeof(words)));
        TRY(hipMemcpy(in, KAT_IN, sizeof(KAT_IN), hipMemcpyHostToDevice));
        TRY(hipMemset(out, 0, sizeof(words)));
        kat_kernel<<<1, 64>>>(in, out);
        TRY(hipGetLastError());
        overload_kernel<<<N_OVERLOAD / 256, 256>>>(bad);
        TRY(hipGetLastError());
        TRY(hipMemcpy(words, out, sizeof(words), hipMemcpyDeviceToHost));
        TRY(hipMemcpy(&miss, bad, 8, hipMemcpyDeviceToHost));
        unsigned wrong = 0;
        std::printf("noise_domain kat: words");
        for (int v = 0; v < 3; ++v)
            for (int k = 0; k < 8; ++k) {
                std::printf(" %08x", words[8 * v + k]);
                wrong += words[8 * v + k] != KAT_OUT[v][k & 3];
            }
        std::printf("; known-answer mismatches %u; overloads %u inputs, mismatches %llu\n", wrong, N_OVERLOAD, miss);
        if (int rc = write_file(dir, "kat.u32", words, sizeof(words))) return rc;
        return (wrong || miss) ? 1 : 0;
    }

    if (mode == "radius" || mode == "trig" || mode == "product") {
        float *radius = nullptr, *cs = nullptr, *sn = nullptr;
        TRY(hipMalloc(&radius, sizeof(float) * N_RADIUS));
        TRY(hipMalloc(&cs, sizeof(float) * N_ANGLE));
        TRY(hipMalloc(&sn, sizeof(float) * N_ANGLE));
        if (int rc = fill_tables(radius, cs, sn, bad)) return rc;
        if (mode == "radius") {
            TRY(hipMemcpy(&miss, bad, 8, hipMemcpyDeviceToHost));
            std::printf("noise_domain radius: %u inputs, bm_u1_mul mismatches %llu\n", N_RADIUS, miss);
            if (int rc = save(dir, "radius.f32", radius, N_RADIUS)) return rc;
            return miss ? 1 : 0;
        }
        if (mode == "trig") {
            std::printf("noise_domain trig: %u inputs\n", N_ANGLE);
            if (int rc = save(dir, "cos.f32", cs, N_ANGLE)) return rc;
            return save(dir, "sin.f32", sn, N_ANGLE);
        }
        const uint32_t pairs = 4u + N_HASHED;
        TRY(hipMemset(bad, 0, 8));
        product_kernel<<<(pairs + 255u) / 256u, 256>>>(radius, cs, sn, pairs, bad);
        TRY(hipGetLastError());
        TRY(hipMemcpy(&miss, bad, 8, hipMemcpyDeviceToHost));
        std::printf("noise_domain product: %u pairs, mismatches %llu\n", pairs, miss);
        return miss ? 1 : 0;
    }

    if (mode == "stream") {
        if (argc != 8) { std::printf("noise_domain stream: needs DIR SEED SOLVE FIRST N R\n"); return 2; }
        const uint64_t seed = std::strtoull(argv[3], nullptr, 0), first = std::strtoull(argv[5], nullptr, 0);
        const uint64_t solve = std::strtoull(argv[4], nullptr, 0), n = std::strtoull(argv[6], nullptr, 0);
        const uint64_t R = std::strtoull(argv[7], nullptr, 0);
        if (solve >> 32 || n < 1 || n > (1u << 20) || R < 1 || R > 1024) { std::printf("noise_domain stream: out of range\n"); return 2; }
        const size_t count = (size_t)n * R * 4;
        float* out = nullptr;
        TRY(hipMalloc(&out, sizeof(float) * count));
        stream_kernel<<<(unsigned)((n * R + 255) / 256), 256>>>(out, first, (uint32_t)n, (uint32_t)R, (uint32_t)solve,
                                                                  (uint32_t)seed, (uint32_t)(seed >> 32));
        TRY(hipGetLastError());
        TRY(hipDeviceSynchronize());
        std::printf("noise_domain stream: %zu floats\n", count);
        return save(dir, "stream.f32", out, count);
    }

    std::printf("noise_domain: unknown mode %s\n", mode.c_str());
    return 2;
}
