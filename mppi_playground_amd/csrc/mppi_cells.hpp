// mppi_cells.hpp — the tagged 8-byte cell: the only hand-off between the blocks of one launch and between devices.
// Part of the MPPI.forward() hot path for gfx950; see mppi_handle.hpp for the map of the files.  Device-only.
#pragma once
#include <hip/hip_runtime.h>

namespace mppi {
// THE PROTOCOL.  A cell is one aligned 64-bit word {32-bit tag (high), 32-bit payload (low)}.  The writer stores both with
// ONE relaxed store; a reader polls with relaxed loads until the tag is the one it waits for and takes the payload out of
// THE SAME loaded word.  An aligned 8-byte access is never torn, so data and "ready" cannot be seen apart (the idea of
// RCCL's low-latency protocol) and NO FENCE is needed: nothing but the word itself is handed over, so no ordering against
// any other access is relied on (a device-scope fence per block costs far more than a kernel boundary on this part).  A
// wider payload travels as several cells, each complete in itself.  Buffers start out zeroed and no writer uses tag 0; a
// buffer is reused by moving on to the next tag (next_tag in mppi_handle.hpp; the Brent search numbers its probes above a
// per-launch base), never by clearing it.  How far a writer may run ahead (double-buffering) and how a reader waits
// (sleep, time-out, back-off: measured per site) are each user's own.  Scope: agent between the blocks of one device (the
// default), system for cells in a peer's memory.
__device__ __forceinline__ unsigned long long cell_pack(unsigned tag, unsigned bits) { return ((unsigned long long)tag << 32) | (unsigned long long)bits; }
__device__ __forceinline__ unsigned long long cell_pack(unsigned tag, float v) { return cell_pack(tag, __float_as_uint(v)); }
__device__ __forceinline__ unsigned cell_tag(unsigned long long cell) { return (unsigned)(cell >> 32); }
__device__ __forceinline__ float cell_f32(unsigned long long cell) { return __uint_as_float((unsigned)cell); }
// a double that travelled as two cells: its low and its high word
__device__ __forceinline__ double cell_f64(unsigned long long lo, unsigned long long hi) { return __longlong_as_double((long long)((hi << 32) | (lo & 0xFFFFFFFFull))); }
template <int SCOPE = __HIP_MEMORY_SCOPE_AGENT>
__device__ __forceinline__ void cell_store(unsigned long long* p, unsigned long long cell) { __hip_atomic_store(p, cell, __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE = __HIP_MEMORY_SCOPE_AGENT>
__device__ __forceinline__ unsigned long long cell_load(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

}  // namespace mppi
