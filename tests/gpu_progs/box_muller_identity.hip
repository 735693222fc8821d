// box_muller_identity — the operand forms of box_muller (csrc/philox.hpp: bm_u1_fma, bm_angle) against the forms they
// replace, restated literally here, bit for bit over EVERY input that can reach them:
//   u1:    all 2^24 values of a >> 8, each with the low byte 0x00 and 0xff (the low byte must be ignored); the
//          four-instruction form some callers keep (bm_u1_mul) is held to the same restatement;
//   angle: all 2^23 values of b >> 9, each with the low nine bits 0 and all ones.
// One launch each.  Prints the mismatch counts; exit status 1 unless all are 0.
// Build (tests/test_gpu_box_muller_identity.py does it): hipcc + the library's own flags without -shared / -fPIC,
// -I mppi_playground_amd/csrc.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <stdint.h>
#include "philox.hpp"

__device__ __forceinline__ float old_u1(uint32_t a) { return (float)((a >> 8) + 1u) * (1.0f / 16777216.0f); }
__device__ __forceinline__ float old_angle(uint32_t b) { return __uint_as_float(0x3f800000u | (b >> 9)); }

__global__ __launch_bounds__(256) void check_u1(unsigned long long* bad) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;  // a >> 8: the grid covers 2^24 exactly
    unsigned miss = 0, miss_mul = 0;
    for (uint32_t low = 0; low <= 0xffu; low += 0xffu) {
        const uint32_t a = (n << 8) | low;
        miss += __float_as_uint(old_u1(a)) != __float_as_uint(mppi::bm_u1_fma(a));
        miss_mul += __float_as_uint(old_u1(a)) != __float_as_uint(mppi::bm_u1_mul(a));
    }
    if (miss) atomicAdd(bad, (unsigned long long)miss);
    if (miss_mul) atomicAdd(bad + 2, (unsigned long long)miss_mul);
}

__global__ __launch_bounds__(256) void check_angle(unsigned long long* bad) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;  // b >> 9: the grid covers 2^23 exactly
    unsigned miss = 0;
    for (uint32_t low = 0; low <= 0x1ffu; low += 0x1ffu) {
        const uint32_t b = (n << 9) | low;
        miss += __float_as_uint(old_angle(b)) != __float_as_uint(mppi::bm_angle(b));
    }
    if (miss) atomicAdd(bad + 1, (unsigned long long)miss);
}

#define TRY(x)                                                                              \
    do {                                                                                    \
        const hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) { std::printf("box_muller_identity: %s: %s\n", #x, hipGetErrorString(e_)); return 2; } \
    } while (0)

int main() {
    unsigned long long* bad = nullptr;
    TRY(hipMalloc(&bad, 24));
    TRY(hipMemset(bad, 0, 24));
    check_u1<<<(1u << 24) / 256, 256>>>(bad);
    TRY(hipGetLastError());
    check_angle<<<(1u << 23) / 256, 256>>>(bad);
    TRY(hipGetLastError());
    unsigned long long b[3] = {~0ull, ~0ull, ~0ull};
    TRY(hipMemcpy(b, bad, 24, hipMemcpyDeviceToHost));
    std::printf("box_muller_identity: u1 %u inputs, mismatches %llu (four-instruction form: %llu); angle %u inputs, mismatches %llu\n",
                2u << 24, b[0], b[2], 2u << 23, b[1]);
    return (b[0] | b[1] | b[2]) ? 1 : 0;
}
