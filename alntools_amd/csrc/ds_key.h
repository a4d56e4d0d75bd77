// ---- ecdownsample's key: the 128 bits of Philox4x32-10 that rank the reads of a sample (included by ecb.hip behind boot_draw.h, before
// downsample.inc) --------------------------------------------------------------------------------------------------------------------------
// Plain C++ as well as HIP: a host program that includes this file and boot_draw.h alone computes the key and the digits of any
// (seed, s, r) as the kernels do (tests/test_ecdownsample.py builds one).  The rule is include/ecb_downsample.h's.
#ifndef ECB_DS_KEY_H
#define ECB_DS_KEY_H

#include "boot_draw.h"

// the key of read r of sample s: v[3] is the most significant word (o3), v[0] the least (o0); counter (r, 0, s, 1) -- ecboot's is (j, 0, b, 0)
typedef BsPhilox DsKey;
BS_HD DsKey ds_key(uint64_t seed, uint32_t s, uint32_t r) { return bs_philox(r, 0u, s, 1u, (uint32_t)seed, (uint32_t)(seed >> 32)); }
// word w of a key counted from the most significant (0 .. 3), by selects: a key lives in registers and d is a loop variable
BS_HD uint32_t ds_word(const DsKey& k, uint32_t w) { return w == 0u ? k.v[3] : w == 1u ? k.v[2] : w == 2u ? k.v[1] : k.v[0]; }
// 8-bit digit d of a key: 0 = the most significant, 15 = the least
BS_HD uint32_t ds_digit(const DsKey& k, uint32_t d) { return (ds_word(k, d >> 2) >> (8u * (3u - (d & 3u)))) & 255u; }
// the bits of word w (from the most significant) that lie in the first nd digits of a key
BS_HD uint32_t ds_mask(uint32_t w, uint32_t nd) {
    const uint32_t in = nd <= 4u * w ? 0u : nd - 4u * w;
    return in >= 4u ? 0xFFFFFFFFu : in == 0u ? 0u : 0xFFFFFFFFu << (32u - 8u * in);
}
// p with digit d set to b (the digit was 0)
BS_HD void ds_set_digit(DsKey& p, uint32_t d, uint32_t b) { p.v[3u - (d >> 2)] |= b << (8u * (3u - (d & 3u))); }
// whether the first nd digits of k are those of p
BS_HD bool ds_match(const DsKey& k, const DsKey& p, uint32_t nd) {
    bool same = true;
    for (uint32_t w = 0; w < 4u; ++w) same = same && ((ds_word(k, w) ^ ds_word(p, w)) & ds_mask(w, nd)) == 0u;
    return same;
}
// whether the first nd digits of k, read as one number, are at most those of p
BS_HD bool ds_at_most(const DsKey& k, const DsKey& p, uint32_t nd) {
    for (uint32_t w = 0; w < 4u; ++w) {
        const uint32_t m = ds_mask(w, nd), a = ds_word(k, w) & m, b = ds_word(p, w) & m;
        if (a != b) return a < b;
    }
    return true;
}

#endif  // ECB_DS_KEY_H
