// mppi_colored.hpp — The scalar rule of the temporally correlated (AR(1)) sampling noise: the standard normals of one
// (sample, control dimension) pass through a first-order filter along the horizon before they are scaled by sigma.
//     z[0] = xi[0],   z[t] = beta * z[t-1] + alpha * xi[t],   alpha = sqrt(1 - beta^2),   eps[t] = z[t] * s[t]
// The start is stationary: every z[t] keeps variance 1 (so s[t] stays the marginal standard deviation of step t) and the
// lag-1 correlation is beta.
// Plain C++ as well as HIP: the CPU suite compiles this text with g++ and holds it against numpy.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MPPI_HOST_DEVICE __host__ __device__
#else
#define MPPI_HOST_DEVICE
#endif

namespace mppi {

// alpha of an fp32 beta in [0, 1): the square root is taken in double and rounded once (formed on the host, handed to the
// kernels in a table next to beta)
inline float colored_alpha(float beta) { return (float)sqrt(1.0 - (double)beta * (double)beta); }

// z[t] from z[t-1] and the fresh normal xi[t].  fp32, one rounding per operation: the two products, then the sum (the library
// is built with -ffp-contract=off).  beta = 0, alpha = 1 returns xi itself.
MPPI_HOST_DEVICE inline float colored_step(float z_prev, float xi, float beta, float alpha) {
    const float carried = beta * z_prev;
    const float fresh = alpha * xi;
    return carried + fresh;
}

}  // namespace mppi
