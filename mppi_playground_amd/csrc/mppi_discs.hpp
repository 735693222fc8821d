// mppi_discs.hpp — The scalar pieces of the moving-disc penalty (MPPI_MODEL_NAV2D_DISCS; include/mppi_hip.h, mppi_set_discs,
// states the rule): one row of the table holds MPPI_MAX_DISCS discs {cx, cy, r2, w}; a position inside disc j
// (squared distance <= r2, the squared radius the caller formed) pays w.  Penalties add up over the discs in slot order.
// Plain C++ as well as HIP: the CPU suite compiles this text with g++ and holds it against numpy (tests/discs_ref.py),
// and a model other than nav2d can reuse it.
// FUSE = false (math level 0): every operation rounds once to fp32 — two products and one add — so a numpy fp32
// restatement reproduces the device's bits.  FUSE = true (the fast levels): d2 = fma(dx, dx, dy * dy), spelled out, so that
// every copy of the horizon loop forms the same bits whatever the compiler would have contracted.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MPPI_DISC_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define MPPI_DISC_HOST_DEVICE inline
#endif

namespace mppi {

constexpr int DISC_FLOATS = 4;  // {cx, cy, r2, w}
constexpr int DISC_ROW = DISC_FLOATS * 8;  // floats per step of the padded table (8 = MPPI_MAX_DISCS)
// an unused slot of the padded table: r2 = -1 is below every squared distance, w = 0 pays nothing even if it were hit
constexpr float DISC_PAD_R2 = -1.0f, DISC_PAD_W = 0.0f;

struct alignas(16) Disc { float cx, cy, r2, w; };  // 16 bytes, 16-byte aligned (the rows are, in LDS and in the handle's buffer): one read

// squared distance of (x, y) from the disc's centre
template <bool FUSE>
MPPI_DISC_HOST_DEVICE float disc_d2(float x, float y, const Disc& k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float dx = x - k.cx, dy = y - k.cy;
    if (FUSE) return fmaf(dx, dx, dy * dy);
    const float px = dx * dx, py = dy * dy;
    return px + py;
}

// pen + (the disc's penalty when (x, y) lies in it)
template <bool FUSE>
MPPI_DISC_HOST_DEVICE float disc_add(float pen, float x, float y, const Disc& k) {
    return pen + (disc_d2<FUSE>(x, y, k) <= k.r2 ? k.w : 0.0f);
}

// the penalty of one row: discs 0 .. n-1 of `row` ([8][4], 16-byte aligned), in slot order
template <bool FUSE>
MPPI_DISC_HOST_DEVICE float disc_row_penalty(const float* row, int n, float x, float y) {
    float pen = 0.0f;
    for (int j = 0; j < n; ++j) {
        const Disc k = *reinterpret_cast<const Disc*>(row + DISC_FLOATS * j);
        pen = disc_add<FUSE>(pen, x, y, k);
    }
    return pen;
}

// ------------------------------------------------------------------------------------------------ the soft rule
// The graded skirt of the soft disc models (include/mppi_hip.h, mppi_set_disc_softness, states the rule): inside the disc
// (the hard rule's own compare, d2 <= r2) the penalty is w; outside it is w * max(a - b * d2 / r2, 0), linear in d2 from
// skirt * w at the rim to 0 at reach * r.  a and b are the two launch-uniform coefficients the host formed from (reach, skirt).
// FUSE = false: every operation rounds on its own, with the IEEE quotient, so a numpy fp32 restatement reproduces the bits.
// FUSE = true: every fused operation is spelled out (fmaf), and the quotient is d2 * rcp(r2) — one v_rcp_f32 on the device,
// 1.0f / r2 in a host build.  With a = b = 0 both forms return the hard rule's bits (f is 0 or 1, w * 1 is exact).
MPPI_DISC_HOST_DEVICE float disc_rcp(float r2) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(r2);
#else
    return 1.0f / r2;
#endif
}

// pen + w * (1 inside the disc, the ramp outside it)
template <bool FUSE>
MPPI_DISC_HOST_DEVICE float disc_add_soft(float pen, float x, float y, const Disc& k, float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float d2 = disc_d2<FUSE>(x, y, k);
    if (FUSE) {
        const float q = d2 * disc_rcp(k.r2);
        const float ramp = fmaxf(fmaf(-b, q, a), 0.0f);
        return fmaf(k.w, d2 <= k.r2 ? 1.0f : ramp, pen);
    }
    const float q = d2 / k.r2;
    const float bq = b * q;
    const float ramp = fmaxf(a - bq, 0.0f);
    const float wf = k.w * (d2 <= k.r2 ? 1.0f : ramp);
    return pen + wf;
}

// the soft penalty of one row: discs 0 .. n-1 of `row`, in slot order
template <bool FUSE>
MPPI_DISC_HOST_DEVICE float disc_row_penalty_soft(const float* row, int n, float x, float y, float a, float b) {
    float pen = 0.0f;
    for (int j = 0; j < n; ++j) {
        const Disc k = *reinterpret_cast<const Disc*>(row + DISC_FLOATS * j);
        pen = disc_add_soft<FUSE>(pen, x, y, k, a, b);
    }
    return pen;
}

}  // namespace mppi
