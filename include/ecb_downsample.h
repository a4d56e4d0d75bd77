/*
 * ecb_downsample.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that thins the samples of a .bin to a read
 * depth: n of a sample's M reads drawn WITHOUT replacement (ecdownsample).
 * Same conventions as ecb.h: plain C types, the caller owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL)
 * explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_DOWNSAMPLE_H
#define ECB_DOWNSAMPLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Downsample (ABI 4, additive).
 * In (device memory in ecb_downsample_device, host memory in ecb_downsample):
 *   N        CSC over (EC, sample) as ecb_count_alignments takes it, and checked the same way: int32 column pointers [n_samples + 1] from
 *            0 to nnz_n, never falling; int32 EC indices [nnz_n] below n_ecs; int32 counts [nnz_n] >= 0.  An EC listed twice in a column
 *            is two entries.
 *   target   int64 [n_samples].      seed   any 64 bits.
 * The rule.  For sample s, its entries in column order have the counts c_0 .. c_(k-1); M_s is their sum and cum_j = c_0 + .. + c_j.  The
 * reads of s are numbered 0 .. M_s - 1 in entry order: read r belongs to the entry j with cum_(j-1) <= r < cum_j.  n_s = target[s].
 *   n_s < 0 or n_s >= M_s   every count of the column is copied.
 *   n_s == 0                every count of the column becomes 0.
 *   otherwise               read r has the 128-bit key  o3 * 2^96 + o2 * 2^64 + o1 * 2^32 + o0  with
 *                             (o0, o1, o2, o3) = Philox4x32-10(counter = (r, 0, s, 1), key = (seed & 0xffffffff, seed >> 32)),
 *                           Random123's constants and round (csrc/boot_draw.h; the fourth counter word 1 keeps the stream apart from
 *                           ecboot's, which is 0).  The n_s reads with the smallest keys stay; the output count of an entry is the number
 *                           of its reads that stay.
 * There is no tie rule and none is needed: for a fixed key Philox is a bijection of its counter, and the reads of one sample differ in
 * the first counter word, so two reads of a sample never share a key.  The kernels rely on this (a radix select on the key's digits ends
 * with buckets of one read at the latest).
 * The result is a function of (N, target, seed) alone: not of the targets of the other samples, of batching, of launch geometry, of what
 * scratch memory held, or of the entry point.  Counts are integers, and integer atomics are exact in any order.
 * Out (device / host memory as the inputs):
 *   out_data_n   int32 [nnz_n]: one count per input entry, at the entry's own place, zeros included -- indptr_n and indices_n stay valid
 *                for it; compaction is ecb_select's job.
 *   in_total     int64 [n_samples]: M_s.  May be NULL.
 *   out_total    int64 [n_samples]: the reads of s that stay.  May be NULL.
 * Refusals, every one of which leaves every output untouched:
 *   ECB_ERR_ARG       indptr_n, target or -- where nnz_n > 0 -- indices_n, data_n or out_data_n is NULL; a pointer that is not aligned to
 *                     its element (4 bytes, 8 for target and the totals); an output shares a byte with an input or with another output.
 *   ECB_ERR_CONTRACT  a malformed N (above).
 *   ECB_ERR_LIMIT     n_ecs, n_samples or nnz_n beyond the .bin format's int32 limits; M_s >= 2^31 for a sample with 0 <= n_s < M_s (a
 *                     read's number is one counter word; such a column with n_s < 0 is copied like any other); the samples with
 *                     0 < n_s < M_s and M_s above 2048 together hold 2^31 or more stretches of 4096 reads (the grid of the passes over
 *                     them: beyond 2^43 reads).
 * n_samples = 0 and nnz_n = 0 are no errors.
 * ecb_downsample_device: every array, target included, is in device memory.  ecb_downsample: the same on HOST arrays (the library
 * allocates and frees its own device buffers). */
int ecb_downsample_device(int device, uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n, const void* d_indices_n,
                          const void* d_data_n, const void* d_target, uint64_t seed, void* d_out_data_n, void* d_in_total, void* d_out_total);
int ecb_downsample(int device, uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n, const int32_t* indices_n,
                   const int32_t* data_n, const int64_t* target, uint64_t seed, int32_t* out_data_n, int64_t* in_total, int64_t* out_total);

#ifdef __cplusplus
}
#endif
#endif /* ECB_DOWNSAMPLE_H */
