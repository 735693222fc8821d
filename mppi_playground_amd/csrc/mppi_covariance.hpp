// mppi_covariance.hpp — The scalar rule of the covariance adaptation (the sketch at mppi.py:400-418): one column of the
// per-step sigma table moves towards the weighted variance of that column's clamped actions.
// Plain C++ as well as HIP: the CPU suite compiles this text with g++ and holds it against numpy.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MPPI_HOST_DEVICE __host__ __device__
#else
#define MPPI_HOST_DEVICE
#endif

namespace mppi {

// s^2 <- (1 - rate) * s^2 + rate * (var + floor), s clamped into [smin, smax]; returns s.  fp32, one rounding per
// operation (the library is built with -ffp-contract=off).  rate = 1 is the reference's sketch (covariance = var + 1e-6,
// mppi.py:402-411); rate = 0 returns sqrt(s2_old): the table entry itself when s2_old = fl(s * s) (a correctly rounded
// square root undoes a rounded square in binary floating point).  `var` must be finite (the caller skips a voided solve).
MPPI_HOST_DEVICE inline float covariance_step(float s2_old, float var, float rate, float floor, float smin, float smax) {
    const float target = var + floor;
    const float s2 = (1.0f - rate) * s2_old + rate * target;
    const float s = sqrtf(s2);
    return fminf(fmaxf(s, smin), smax);
}

}  // namespace mppi
