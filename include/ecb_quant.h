/*
 * ecb_quant.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that estimates abundances from a .bin: the EM whose
 * one iteration is the reference's multiply / normalize_reads / sum.  Same conventions as ecb.h: plain C types, the caller owns every
 * buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL) explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_QUANT_H
#define ECB_QUANT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ecquant (ABI 4, additive): EM abundance estimates of a .bin -- iterated, what the reference's AlignmentPropertyMatrix.multiply(axis=2),
 * normalize_reads(axis=READ) and sum(axis=READ) compute (AlignmentPropertyMatrix.py:277-384).  A: CSR over (EC, locus), values = haplotype
 * bitmasks; N: CSC over (EC, sample); sample: -1 = all columns pooled, or one column -- all exactly as ecb_count_alignments takes them, and
 * w[e] is the weight of row e as defined there.  scale, theta_in: float64 [n_haps x n_loci] row-major, either may be NULL (scale: 1
 * everywhere; theta_in: theta_0[h, t] = aln[h, t] of ecb_count_alignments).
 *   one step theta -> theta':   phi = theta * scale (entry by entry)
 *                               d[e] = the sum of phi[h, t] over every set bit h of every non-zero (e, t) of row e
 *                               r[e] = w[e] / d[e] when d[e] > 0, else 0
 *                               theta'[h, t] = phi[h, t] * (the sum of r[e] over the rows e whose non-zero at t has bit h)
 *   delta_k = the sum over (h, t) of |theta_{k+1} - theta_k|;   W = the sum of w[e] over the rows that hold a set bit
 * Steps are applied until the first k with delta_k <= tol * W (converged = 1) or until max_iters steps have been applied; max_iters = 0
 * returns theta_0.  theta stays in read units whatever scale is: the sum of theta' is `explained`.
 * Outputs: theta float64 [n_haps x n_loci] row-major (required); and on the HOST, each may be NULL: n_iter = steps applied, delta = the last
 * delta_k (0 when no step ran), explained = the sum of w[e] over the rows with d[e] > 0 in the last step (0 when no step ran), converged.
 * The result is a function of the inputs alone: no float atomics, every sum in a fixed order, the stop at exactly the k defined above.
 * Refused with every output untouched: what ecb_count_alignments refuses, with its codes (a malformed A or N, an unknown sample:
 * ECB_ERR_CONTRACT; nnz_a of 2^30 or more, 2^32 set bits or more: ECB_ERR_LIMIT); an entry of scale or theta_in that is NaN, infinite or negative:
 * ECB_ERR_CONTRACT; a tol that is NaN or negative, a null theta: ECB_ERR_ARG.  n_ecs = 0 or nnz_a = 0 is no error: theta = 0, n_iter = 0,
 * converged = 1.
 * ecb_quantify_device: the arrays in device memory;  ecb_quantify: the same on HOST arrays (the library allocates and frees its own device
 * buffers). */
int ecb_quantify_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                        const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                        const void* d_indices_n, const void* d_data_n, int64_t sample, const void* d_scale, const void* d_theta_in,
                        uint32_t max_iters, double tol, void* d_theta, uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged);
int ecb_quantify(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                 const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                 const int32_t* indices_n, const int32_t* data_n, int64_t sample, const double* scale, const double* theta_in,
                 uint32_t max_iters, double tol, double* theta, uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged);

#ifdef __cplusplus
}
#endif

/* the same EM with EMASE's hierarchical models over a gene grouping (ecb_quantify_model / ecb_quantify_model_device): a header of its own */
#include "ecb_quant_model.h"
/* ... and one EM per cell of a multisample N, batched, the result sparse (ecb_cell_support* / ecb_quantify_cells*): likewise */
#include "ecb_quant_cells.h"
/* ... and the hierarchical models per cell (ecb_quantify_cells_model*): likewise */
#include "ecb_quant_cells_model.h"
/* ... and the posterior probability of every alignment at a given theta (ecb_posterior*): likewise */
#include "ecb_quant_post.h"
/* ... and bootstrap replicates of N, the mean and standard deviation of their estimates (ecb_resample* / ecb_quantify_bootstrap*): likewise */
#include "ecb_quant_boot.h"

#endif /* ECB_QUANT_H */
