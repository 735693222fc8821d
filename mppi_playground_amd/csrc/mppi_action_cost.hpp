// mppi_action_cost.hpp — The scalar pieces of the opt-in control-cost term (the `action_costs` the reference fills at
// mppi.py:294-316 and leaves out of the cost sum at :330-336): the inverse variance of one column, the per-column factor
// g = mean * inv, one accumulate step of A = sum g * U, and the final cost = c0 + kappa * A.
// Plain C++ as well as HIP: the CPU suite compiles this text with g++ (-ffp-contract=off) and holds it against numpy.
// Every operation rounds once to fp32: a separate multiply and add, never an FMA, so that a numpy fp32 restatement
// reproduces the device's bits.
#pragma once

#if defined(__HIPCC__)
#define MPPI_AC_HOST_DEVICE __host__ __device__
#else
#define MPPI_AC_HOST_DEVICE
#endif

namespace mppi {

// inv[t] of column (t, k) with standard deviation `s`: 0 for t = 0 (mppi.py:135-136 and :413 fill rows 1..T-1 only; row
// 0 of `_inv_covariance` stays zero), 1 / (s * s) otherwise.  `s` must be > 0 (the set-up path checks).
MPPI_AC_HOST_DEVICE inline float action_cost_inv(int t, float s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (t == 0) return 0.0f;
    const float s2 = s * s;
    return 1.0f / s2;
}

// g[t][k] = mean[t][k] * inv[t][k] (mppi.py:313: mean_action_seq[t] @ inv_covariance[t], diagonal)
MPPI_AC_HOST_DEVICE inline float action_cost_g(float mean, float inv) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return mean * inv;
}

// one step of the sequential sum over (t, k): A <- A + g * u, the product rounded before the sum
MPPI_AC_HOST_DEVICE inline float action_cost_accumulate(float A, float g, float u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = g * u;
    return A + p;
}

// kappa = action_cost_weight * lambda (mppi.py:335: self._lambda * action_costs; the weight is the paper's 1 - alpha)
MPPI_AC_HOST_DEVICE inline float action_cost_kappa(float weight, float lambda) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return weight * lambda;
}

// cost = c0 + kappa * A
MPPI_AC_HOST_DEVICE inline float action_cost_total(float c0, float kappa, float A) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = kappa * A;
    return c0 + p;
}

}  // namespace mppi
