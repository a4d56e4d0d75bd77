/*
 * ecb_select.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that keeps a part of a .bin: the reads of one
 * class and the samples that still count enough of them.  Same conventions as ecb.h: plain C types, the caller owns every buffer, 0 = OK,
 * < 0 = an ECB_ERR_* code that ecb_last_error(NULL) explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_SELECT_H
#define ECB_SELECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ecselect (ABI 4, additive): rows of A and columns of N pulled out of one .bin -- the selection of the reference's
 * AlignmentPropertyMatrix.get_unique_reads / pull_alignments_from (AlignmentPropertyMatrix.py:386-427) and the cell threshold of its
 * bam2ec --multisample (bam_utils_multisample.py:596-636).  A: CSR over (EC, locus), values = haplotype bitmasks; N: CSC over (EC, sample).
 * With bits(e) = the set bits of all of row e's masks and nz(e) = its non-zeros whose mask is not 0, in this order:
 *   1. row_class   0: every row is in class (empty ones too);  1: bits == 1 (allele-unique);  2: nz == 1 (locus-unique);  3: nz >= 2 (multi)
 *   2. sample_keep uint8 [n_samples], not 0 = the sample is named; NULL: all are
 *   3. min_count   < 0: every named sample stays; otherwise total[s] = the sum of column s of N over the rows in class (int64), and a named
 *                  sample stays when total[s] >= max(min_count, 1)
 *   4. an entry of N stays when its row is in class, its sample stays and its count is above 0; entries are copied one for one, in their
 *      order within the column (an EC listed twice in a column stays listed twice)
 *   5. a row stays when it is in class and an entry of it stays; rows keep their order and are renumbered from 0; a row of A that stays is
 *      copied whole, stored 0 masks included
 * The input must be well formed as for ecb_count_alignments, otherwise ECB_ERR_CONTRACT and no output is written: A's row pointers from 0 to
 * nnz_a, never falling; columns below n_loci, strictly ascending within a row; no mask bit at or above n_haps <= 31 (a mask of 0 is
 * allowed); N's column pointers from 0 to nnz_n, never falling; EC indices below n_ecs; counts >= 0.  A row_class other than 0 .. 3 or a
 * null pointer (sample_keep apart; the index and value arrays of a matrix without entries too): ECB_ERR_ARG.  Sizes beyond the .bin
 * format's int32 limits: ECB_ERR_LIMIT.
 * Outputs, sized by the caller as the inputs (the result is never larger): out_indptr_a n_ecs + 1, out_indices_a / out_data_a nnz_a,
 * out_indptr_n n_samples + 1, out_indices_n / out_data_n nnz_n, out_sample_keep uint8 [n_samples] (1 = the sample stayed; the kept samples
 * are the result's columns, in the input's order).  out_sizes (host) = {n_ecs, nnz_a, n_samples, nnz_n} of the result; only that much of
 * every output is written.  A result without a sample or without a row is no error here.
 * ecb_select_device: every array in device memory (outputs not overlapping the inputs or each other, otherwise ECB_ERR_ARG);  ecb_select:
 * the same on HOST arrays (the library allocates and frees its own device buffers). */
int ecb_select_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples, uint64_t nnz_a, const void* d_indptr_a,
                      const void* d_indices_a, const void* d_data_a, uint64_t nnz_n, const void* d_indptr_n, const void* d_indices_n,
                      const void* d_data_n, int32_t row_class, const void* d_sample_keep, int64_t min_count, void* d_out_indptr_a,
                      void* d_out_indices_a, void* d_out_data_a, void* d_out_indptr_n, void* d_out_indices_n, void* d_out_data_n,
                      void* d_out_sample_keep, uint64_t* out_sizes);
int ecb_select(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples, uint64_t nnz_a, const int32_t* indptr_a,
               const int32_t* indices_a, const int32_t* data_a, uint64_t nnz_n, const int32_t* indptr_n, const int32_t* indices_n,
               const int32_t* data_n, int32_t row_class, const uint8_t* sample_keep, int64_t min_count, int32_t* out_indptr_a,
               int32_t* out_indices_a, int32_t* out_data_a, int32_t* out_indptr_n, int32_t* out_indices_n, int32_t* out_data_n,
               uint8_t* out_sample_keep, uint64_t* out_sizes);

#ifdef __cplusplus
}
#endif
#endif /* ECB_SELECT_H */
