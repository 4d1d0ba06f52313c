// The sort key of the training subsample (include/doda_subsample.h), defined ONCE: Philox-4x32-10 (Salmon et al., "Parallel random
// numbers: as easy as 1, 2, 3", SC'11) with the key (seed_lo, seed_hi) and the counter (j, 0, 0, 0); the key of point j is output
// word 0.  Counter based: any point's key is recomputed wherever it is needed, so no pass stores one.  tests/subsample_cases.py
// restates it in numpy.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DODA_SUBSAMPLE_HD __host__ __device__
#else
#define DODA_SUBSAMPLE_HD
#endif

DODA_SUBSAMPLE_HD static inline uint32_t subsample_key(uint32_t seed_lo, uint32_t seed_hi, uint32_t j) {
    uint32_t c0 = j, c1 = 0u, c2 = 0u, c3 = 0u, k0 = seed_lo, k1 = seed_hi;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}
