// Host build of the in-loop heading wrap of the FAST kinematic models (mppi_models.inc: wrap_inc_f), its mppi::strict and
// mppi::fused copies.  g++ ignores the `#pragma clang fp contract(fast)` of the fused copy, so both are built without
// contraction here; wrap_inc_f holds no contractible a * b + c (explicit FMA, the product feeds floor), so the device's
// fused compilation performs the same operations.  TEST-ONLY (tests/test_wrap_inc_host.py).
#include <cstdint>

#include "../../mppi_playground_amd/csrc/mppi_models.hpp"

extern "C" void probe_wrap_inc(const float* x, float* strict_out, float* fused_out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        strict_out[i] = mppi::strict::wrap_inc_f(x[i]);
        fused_out[i] = mppi::fused::wrap_inc_f(x[i]);
    }
}
