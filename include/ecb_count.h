/*
 * ecb_count.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that reads a .bin back instead of building or
 * rewriting one.  Same conventions as ecb.h: plain C types, the caller owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that
 * ecb_last_error(NULL) explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_COUNT_H
#define ECB_COUNT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* count-alignments (ABI 4, additive): per-target read counts of a .bin -- what the reference's AlignmentPropertyMatrix.count_alignments and
 * count_unique_reads return (AlignmentPropertyMatrix.py:429-448) and its report_alignment_counts writes.  A: CSR over (EC, locus), values =
 * haplotype bitmasks; N: CSC over (EC, sample) as the .bin stores it.  w[e] = the sum of row e of N over all samples (sample = -1) or its
 * entry in one column (0 <= sample < n_samples); an EC that N does not list weighs 0, one listed twice in a column has its counts added.
 *   aln[h, t]      = sum of w[e] over the non-zeros (e, t) whose mask has bit h
 *   uniq[h, t]     = the same over the ECs whose masks hold exactly one set bit in the whole row
 *   locus_uniq[t]  = sum of w[e] over the ECs with exactly one non-zero, at column t (whatever haplotype bits it carries)
 * A mask of 0 is allowed and counts as no non-zero.  Outputs int64, aln / uniq H x T row-major, locus_uniq T; any may be NULL.  The sums are
 * exact integers (no float atomics), the same whatever the order of arrival.
 * The input must be well formed, otherwise ECB_ERR_CONTRACT and no output is written: A as for ecb_apply_mask (row pointers from 0 to nnz_a,
 * never falling; columns below n_loci, strictly ascending within a row; no mask bit at or above n_haps <= 31); N's column pointers from 0 to
 * nnz_n, never falling; EC indices below n_ecs; counts >= 0; sample in [-1, n_samples).  nnz_a of 2^30 or more: ECB_ERR_LIMIT.
 * ecb_count_alignments_device: device pointers;  ecb_count_alignments: the same on HOST arrays (the library allocates and frees its own
 * device buffers). */
int ecb_count_alignments_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                                const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                const void* d_indices_n, const void* d_data_n, int64_t sample, void* d_aln, void* d_uniq, void* d_locus_uniq);
int ecb_count_alignments(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                         const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                         const int32_t* indices_n, const int32_t* data_n, int64_t sample, int64_t* aln, int64_t* uniq, int64_t* locus_uniq);

#ifdef __cplusplus
}
#endif
#endif /* ECB_COUNT_H */
