// kernels_proof.hip — the create-time proof kernels: exhaustive bit-comparisons of the lean quotient, reciprocal and square-root
// forms (fs_device.h) with the correctly rounded operations, over the operand ranges the step relies on.
#include <string.h>

#include "fs_kernels.h"
#include "fs_neighbours.h"

namespace fsd {

// ------------------------------------------------------- proof kernel for div_const
// Enumerates EVERY f32 x with lo <= |x| <= hi (both signs; lo, hi > 0 given as bit patterns) and
// counts those for which div_const_fast(x, c, y) differs bitwise from the correctly rounded x / c.
__global__ __launch_bounds__(FS_BLOCK) void k_verify_constdiv(float c, float y, uint32_t lo_bits, uint32_t hi_bits,
                                                              uint32_t* __restrict__ mismatches) {
    const uint32_t tid = blockIdx.x * FS_BLOCK + threadIdx.x;
    const uint32_t total_threads = gridDim.x * FS_BLOCK;
    uint32_t bad = 0;
    for (uint64_t b = (uint64_t)lo_bits + tid; b <= (uint64_t)hi_bits; b += total_threads) {
        const float x = __uint_as_float((uint32_t)b);                 // positive floats are ordered like their bits
        bad += __float_as_uint(div_const_fast(x, c, y)) != __float_as_uint(__fdiv_rn(x, c)) ? 1u : 0u;
        bad += __float_as_uint(div_const_fast(-x, c, y)) != __float_as_uint(__fdiv_rn(-x, c)) ? 1u : 0u;
    }
    if (bad) atomicAdd(mismatches, bad);
}

static uint32_t f32_bits(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }

void launch_verify_constdiv(hipStream_t st, float c, float y, float lo, float hi, uint32_t* mismatches) {
    hipLaunchKernelGGL(k_verify_constdiv, dim3(256 * 32), dim3(FS_BLOCK), 0, st, c, y, f32_bits(lo), f32_bits(hi), mismatches);
}

// ------------------------------------------------------- proof kernel for rcp_rn_fast / sqrt_rn_fast
// Enumerates EVERY f32 in [lo, hi] (bit patterns; positive) and counts inputs whose lean result
// differs bitwise from the correctly rounded 1.0f / x (which == 0) or __builtin_sqrtf(x) (which == 1).
__global__ __launch_bounds__(FS_BLOCK) void k_verify_unary(int which, uint32_t lo_bits, uint32_t hi_bits,
                                                           uint32_t* __restrict__ mismatches) {
    const uint32_t total_threads = gridDim.x * FS_BLOCK;
    uint32_t bad = 0;
    for (uint64_t b = (uint64_t)lo_bits + blockIdx.x * FS_BLOCK + threadIdx.x; b <= (uint64_t)hi_bits; b += total_threads) {
        const float x = __uint_as_float((uint32_t)b);
        const uint32_t got = __float_as_uint(which == 0 ? rcp_rn_fast(x) : sqrt_rn_fast(x));
        const uint32_t ref = __float_as_uint(which == 0 ? __fdiv_rn(1.0f, x) : sqrt_rn(x));
        bad += got != ref ? 1u : 0u;
    }
    if (bad) atomicAdd(mismatches, bad);
}

void launch_verify_unary(hipStream_t st, int which, float lo, float hi, uint32_t* mismatches) {
    hipLaunchKernelGGL(k_verify_unary, dim3(256 * 32), dim3(FS_BLOCK), 0, st, which, f32_bits(lo), f32_bits(hi), mismatches);
}

}  // namespace fsd
