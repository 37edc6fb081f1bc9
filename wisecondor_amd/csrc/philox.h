// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11; the Random123 constants), one
// routine for host and device: a block of four 32-bit words is a pure function of a 128-bit counter and a
// 64-bit key, so any read of any bin of any trial has its word without a state being carried anywhere.
//   round    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
//   key      (k0, k1) <- (k0 + W0, k1 + W1) between rounds; ten rounds, nine bumps
// Integers only, no table, no memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PX_HD __host__ __device__
#else
#define PX_HD
#endif

#define PX_M0 0xD2511F53u
#define PX_M1 0xCD9E8D57u
#define PX_W0 0x9E3779B9u
#define PX_W1 0xBB67AE85u

PX_HD static inline void px_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)PX_M0 * c0, p1 = (uint64_t)PX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
}

// w[0 .. 3] of counter (c0, c1, c2, c3) under key (k0, k1)
PX_HD static inline void px_block(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        px_round(c0, c1, c2, c3, k0, k1);
        k0 += PX_W0;
        k1 += PX_W1;
    }
    w[0] = c0;
    w[1] = c1;
    w[2] = c2;
    w[3] = c3;
}

// T of f parts per million: a 32-bit word w keeps its read when (uint64) w < T; f = 1 000 000 gives 2^32, which every word is below
PX_HD static inline uint64_t px_threshold(uint32_t f_ppm) { return ((uint64_t)f_ppm << 32) / 1000000ull; }
