// ---- ecboot's draw: Philox4x32-10 and the map of its output onto [0, W) (included by ecb.hip before boot.inc) -----------------------
// Plain C++ as well as HIP: a host program that includes this file alone computes the x of any (seed, b, i, W) as the kernel does
// (tests/test_ecboot.py builds one).  Random123's constants and round; nothing here depends on the device.
#ifndef ECB_BOOT_DRAW_H
#define ECB_BOOT_DRAW_H

#include <stdint.h>

#if defined(__HIPCC__)
#define BS_HD __host__ __device__ __forceinline__
#else
#define BS_HD inline
#endif

struct BsPhilox { uint32_t v[4]; };

// Philox4x32-10(counter c0..c3, key k0 k1): each round c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key
// raised by (0x9E3779B9, 0xBB67AE85) between rounds
BS_HD BsPhilox bs_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    BsPhilox o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}
// the call that serves draws 2 j and 2 j + 1 of replicate b: counter (j, 0, b, 0), key (seed's low word, seed's high word)
BS_HD BsPhilox bs_pair(uint64_t seed, uint32_t b, uint32_t j) { return bs_philox(j, 0u, b, 0u, (uint32_t)seed, (uint32_t)(seed >> 32)); }
// (u W) >> 64 for a W below 2^32: the high word of u's product with W, from two 32 x 32 products
BS_HD uint32_t bs_scale(uint64_t u, uint32_t W) {
    const uint64_t lo = (u & 0xFFFFFFFFull) * W, hi = (u >> 32) * W;
    return (uint32_t)((hi + (lo >> 32)) >> 32);
}
// the x of the even (half = 0) or odd (half = 1) draw of a call
BS_HD uint32_t bs_x(const BsPhilox& o, uint32_t half, uint32_t W) {
    return bs_scale((uint64_t)o.v[2u * half + 1u] << 32 | o.v[2u * half], W);
}
// draw i of replicate b
BS_HD uint32_t bs_draw_x(uint64_t seed, uint32_t b, uint32_t i, uint32_t W) { return bs_x(bs_pair(seed, b, i >> 1), i & 1u, W); }

#endif  // ECB_BOOT_DRAW_H
