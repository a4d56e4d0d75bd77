/*
 * ecb_bundle.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that collapses a .bin's targets into groups.
 * Same conventions as ecb.h: plain C types, the caller owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL)
 * explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_BUNDLE_H
#define ECB_BUNDLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ecbundle (ABI 4, additive): the columns of one .bin collapsed into groups (isoforms into genes) and its rows folded back into ECs -- the
 * reference's AlignmentPropertyMatrix.bundle(reset=True) (AlignmentPropertyMatrix.py:219-275) followed by ecb_combine of the one result.
 * A: CSR over (EC, locus), values = haplotype bitmasks; N: CSC over (EC, sample), as ecb_combine_part holds them.  The group map is a CSR
 * over the loci: map_ptr (uint32, n_loci + 1, from 0 to n_map, never falling), map_idx (uint32, n_map group ids below n_groups, strictly
 * ascending within a locus).  A locus may be in one group, in none (its alignments are dropped) or in several (it counts in each; 65535 at
 * the most, otherwise ECB_ERR_LIMIT).
 *   A'[row, g] = the OR of the row's masks over the loci that are in group g; columns ascending
 * and from there ecb_combine's contract for one part: rows with equal (group, mask) sets are one EC (all rows that lose every alignment
 * share the empty key), ECs are numbered by first appearance, N is summed per (EC, sample), zero sums dropped, CSC.
 * The input must be well formed, otherwise ECB_ERR_CONTRACT and no output is written: A and N as for ecb_combine, the map as above.
 * 2^30 or more (row, group) pairs before the fold, or a summed count beyond int32: ECB_ERR_LIMIT.
 * Outputs: out_indptr_a n_ecs + 1; out_indices_a / out_data_a a_capacity elements each, which the caller sizes: the result has at most
 * min(X, n_ecs * n_groups) non-zeros, X = the sum over the non-zeros of A of the number of groups of their locus (map_ptr[c + 1] -
 * map_ptr[c]); a smaller a_capacity than the fold needs is ECB_ERR_ARG, nothing written.  out_indptr_n n_samples + 1, out_indices_n /
 * out_data_n nnz_n.  out_sizes = {n_ecs, nnz_a, nnz_n} of the result.
 * ecb_bundle_device: every array in device memory (outputs not overlapping the inputs);  ecb_bundle: the same on HOST arrays (the library
 * allocates and frees its own device buffers). */
int ecb_bundle_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples, uint32_t n_groups, uint64_t nnz_a,
                      const void* d_indptr_a, const void* d_indices_a, const void* d_data_a, uint64_t nnz_n, const void* d_indptr_n,
                      const void* d_indices_n, const void* d_data_n, uint64_t n_map, const void* d_map_ptr, const void* d_map_idx,
                      uint64_t a_capacity, void* d_out_indptr_a, void* d_out_indices_a, void* d_out_data_a, void* d_out_indptr_n,
                      void* d_out_indices_n, void* d_out_data_n, uint64_t* out_sizes);
int ecb_bundle(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples, uint32_t n_groups, uint64_t nnz_a,
               const int32_t* indptr_a, const int32_t* indices_a, const int32_t* data_a, uint64_t nnz_n, const int32_t* indptr_n,
               const int32_t* indices_n, const int32_t* data_n, uint64_t n_map, const uint32_t* map_ptr, const uint32_t* map_idx,
               uint64_t a_capacity, int32_t* out_indptr_a, int32_t* out_indices_a, int32_t* out_data_a, int32_t* out_indptr_n,
               int32_t* out_indices_n, int32_t* out_data_n, uint64_t* out_sizes);

#ifdef __cplusplus
}
#endif
#endif /* ECB_BUNDLE_H */
