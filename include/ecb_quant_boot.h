/*
 * ecb_quant_boot.h -- the part of libecb.so's C ABI (include/ecb_quant.h includes this file) that bootstraps ecquant: replicates of N with
 * the reads redrawn on the device, and the mean and standard deviation of their estimates.  Same conventions as ecb.h: plain C types, the
 * caller owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL) explains; these entry points take a device ordinal.
 */
#ifndef ECB_QUANT_BOOT_H
#define ECB_QUANT_BOOT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ecboot's resampling (ABI 4, additive).  N: CSC over (EC, sample) and sample (-1 = all columns pooled, or one column) as
 * ecb_count_alignments takes them; w[e] is the weight of row e as defined there (an EC listed twice adds up), W = the sum of w[e],
 * cum[e] = the inclusive prefix sum in row order.  Replicate b (a uint32, any value) draws W reads.  Draw i, 0 <= i < W:
 *   (o0, o1, o2, o3) = Philox4x32-10(counter = (i >> 1, 0, b, 0), key = (seed & 0xffffffff, seed >> 32))     [Random123's constants]
 *   u = o1 * 2^32 + o0 for even i, o3 * 2^32 + o2 for odd i;   x = (u * W) >> 64
 *   the draw lands on the one row e with cum[e - 1] <= x < cum[e]: a row of weight 0 is never drawn
 * n_b[e] = the number of draws on e; every replicate sums to W exactly.  The result is a function of (N, sample, seed, b) alone: not of
 * which other replicates are drawn, of batching, of launch geometry or of scratch contents (counts are integers: integer atomics are exact
 * in any order).
 * Outputs: a CSC N of n_reps columns, replicates b0 .. b0 + n_reps - 1, that every entry point of the library takes as a multisample N:
 * rep_ptr int32 [n_reps + 1], rep_ec and rep_count int32 [capacity] (rows ascending within a column, no zero counts), *nnz_out (host; may be
 * NULL) = the entries.  rep_ptr and *nnz_out are always written; rep_ec and rep_count only when both are non-null and capacity >= the
 * entries (ecb_cell_support's convention: a first call with capacity 0 sizes them).  n_reps = 0 and W = 0 are no errors.
 * Refused with every output untouched: a malformed N or an unknown sample: ECB_ERR_CONTRACT, as ecb_count_alignments; W >= 2^31 (a count
 * must fit N's int32) or 2^31 entries or more: ECB_ERR_LIMIT; b0 + n_reps > 2^32, a null N or rep_ptr, n_samples = 0: ECB_ERR_ARG.
 * ecb_resample_device: the arrays in device memory;  ecb_resample: the same on HOST arrays. */
int ecb_resample_device(int device, uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n, const void* d_indices_n,
                        const void* d_data_n, int64_t sample, uint64_t seed, uint64_t b0, uint32_t n_reps, void* d_rep_ptr, void* d_rep_ec,
                        void* d_rep_count, uint64_t capacity, uint64_t* nnz_out);
int ecb_resample(int device, uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n, const int32_t* indices_n,
                 const int32_t* data_n, int64_t sample, uint64_t seed, uint64_t b0, uint32_t n_reps, int32_t* rep_ptr, int32_t* rep_ec,
                 int32_t* rep_count, uint64_t capacity, uint64_t* nnz_out);

/* ecboot (ABI 4, additive): A, N, sample, scale, max_iters, tol, n_genes, gene, model as ecb_quantify_model takes them (model 4 is the flat
 * step; gene may then be NULL and is checked when given), budget_bytes as ecb_quantify_cells.  Replicate b, 0 <= b < n_reps, is replicate b
 * of ecb_resample(seed, b0 = 0) quantified as cell b of ecb_quantify_cells / ecb_quantify_cells_model would be: its own theta_0 (the
 * replicate's alignment counts), its own stop, the support rule; dense x_b[h, t] is 0 outside the replicate's support.
 * Moments per (h, t), in replicate order, by one thread:   for b = 0 .. B - 1:  d = x_b - m;  m += d / (b + 1);  M += d * (x_b - m)
 *   mean = m;  sd = sqrt(M / (B - 1)), 0 when B = 1;  tot_mean, tot_sd: the same over y_b[t] = the sum of x_b[h, t], h ascending.
 * Outputs (device memory for the device entry, host memory for the host entry): mean, sd float64 [n_haps x n_loci] row-major (required);
 * each of the others may be NULL: tot_mean, tot_sd float64 [n_loci] (both or neither), reps float64 [n_reps x n_haps x n_loci]; and per
 * replicate, typed as ecb_quantify_cells types them per cell: n_iter uint32, delta float64, explained int64, converged uint8.
 * The running (m, M) carry across batches of replicates: the outputs do not depend on budget_bytes, batching, launch geometry, scratch
 * contents or the entry point.
 * Refused with every output untouched: everything ecb_quantify_model refuses, with its codes; W >= 2^31: ECB_ERR_LIMIT; n_reps = 0, a null
 * mean or sd, a tol that is NaN or negative: ECB_ERR_ARG.  W = 0 or nnz_a = 0 is no error: the moments are 0, converged 1, n_iter 0.
 * Not done: a warm start from the point estimate; a Poisson or binomial-split sampler that needs fewer than W draws; more than one GPU;
 * bootstraps per cell. */
int ecb_quantify_bootstrap_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                                  const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                  const void* d_indices_n, const void* d_data_n, int64_t sample, const void* d_scale, uint32_t max_iters,
                                  double tol, uint64_t budget_bytes, uint32_t n_genes, const void* d_gene, uint32_t model, uint64_t seed,
                                  uint32_t n_reps, void* d_mean, void* d_sd, void* d_tot_mean, void* d_tot_sd, void* d_reps, void* d_n_iter,
                                  void* d_delta, void* d_explained, void* d_converged);
int ecb_quantify_bootstrap(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                           const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                           const int32_t* indices_n, const int32_t* data_n, int64_t sample, const double* scale, uint32_t max_iters,
                           double tol, uint64_t budget_bytes, uint32_t n_genes, const int32_t* gene, uint32_t model, uint64_t seed,
                           uint32_t n_reps, double* mean, double* sd, double* tot_mean, double* tot_sd, double* reps, uint32_t* n_iter,
                           double* delta, int64_t* explained, uint8_t* converged);

#ifdef __cplusplus
}
#endif

#endif /* ECB_QUANT_BOOT_H */
