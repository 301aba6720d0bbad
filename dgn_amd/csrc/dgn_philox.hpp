// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) for host and device:
// the round function and constants of the dropout kernels (dgn_bn_tail.hip, dgn_blk_layer_kernels.hpp keep their own device-only
// copies), with the high halves of the two products taken from 64-bit multiplies so that the host compiles it too.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace dgn {

// c: the 128-bit counter in, the four 32-bit outputs out; (k0, k1): the 64-bit key
__host__ __device__ inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

}  // namespace dgn
