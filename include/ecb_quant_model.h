/*
 * ecb_quant_model.h -- the part of libecb.so's C ABI (include/ecb.h, through ecb_quant.h, which includes this file) that runs ecquant's EM
 * with EMASE's hierarchical models over a gene grouping.  Same conventions as ecb.h: plain C types, the caller owns every buffer, 0 = OK,
 * < 0 = an ECB_ERR_* code that ecb_last_error(NULL) explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_QUANT_MODEL_H
#define ECB_QUANT_MODEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ecquant's models (ABI 4, additive): ecb_quantify with two more inputs -- gene: int32 [n_loci], gene[t] in [0, n_genes), every target in
 * exactly one gene; model: 1 = gene -> allele -> isoform, 2 = gene -> isoform -> allele, 3 = gene -> isoform x allele, 4 = the flat step:
 * the bytes ecb_quantify returns (gene is still checked).  What the reference's normalize_reads(axis=HAPLOGROUP | LOCUS | GROUP,
 * grouping_mat) and bundle(reset=True) compose (AlignmentPropertyMatrix.py:219-275, 340-384).
 *   phi = theta * scale;  Phi_gh = the sum of phi[h, t] over the t of gene g;  Phi_g = the sum of Phi_gh over h;  Phi_t = the sum of
 *   phi[h, t] over h;  S(e) = the (t, h) bits of row e;  D(X) = the sum of phi over a subset X of S(e);  w[e] as for ecb_quantify.
 * The posterior of row e at (t, h), g = gene[t] -- every normalizing sum runs over the members whose own D is positive only:
 *   the gene factor  GF = Phi_g / the sum of Phi_g' over the genes g' with D(S(e) in g') > 0
 *   model 3:  GF * phi[h, t] / D(S(e) in g)
 *   model 1:  GF * Phi_gh / (the sum of Phi_gh' over the h' with D_h' > 0) * phi[h, t] / D_h,   D_h = D({(t', h) in S(e): gene[t'] = g})
 *   model 2:  GF * Phi_t / (the sum of Phi_t' over the t' of g with D_t' > 0) * phi[h, t] / D_t,   D_t = D({(t, h') in S(e)})
 * theta'[h, t] = the sum over rows of w[e] times the posterior;  explained = the sum of w[e] over the rows with D(S(e)) > 0, which the sum
 * of theta' equals up to rounding.  delta, W, the stop, max_iters = 0, theta_in = NULL and the empty inputs: as ecb_quantify.  The
 * reference's factors keep a gene, allele or isoform with D = 0 and Phi > 0 in the denominator and lose that share of the row; where every
 * aligned entry has phi > 0 the two rules are the same.  The result is a function of the inputs alone, as ecb_quantify's is.
 * Refused with every output untouched: a gene[t] outside [0, n_genes): ECB_ERR_CONTRACT (checked on the device); a model outside 1..4, a
 * null gene, n_genes = 0 with n_loci > 0: ECB_ERR_ARG; haplotypes x genes of 2^31 or more: ECB_ERR_LIMIT; everything ecb_quantify refuses,
 * with its codes.
 * ecb_quantify_model_device: the arrays in device memory;  ecb_quantify_model: the same on HOST arrays. */
int ecb_quantify_model_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                              const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                              const void* d_indices_n, const void* d_data_n, int64_t sample, const void* d_scale, const void* d_theta_in,
                              uint32_t max_iters, double tol, uint32_t n_genes, const void* d_gene, uint32_t model, void* d_theta,
                              uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged);
int ecb_quantify_model(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                       const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                       const int32_t* indices_n, const int32_t* data_n, int64_t sample, const double* scale, const double* theta_in,
                       uint32_t max_iters, double tol, uint32_t n_genes, const int32_t* gene, uint32_t model, double* theta,
                       uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged);

#ifdef __cplusplus
}
#endif
#endif /* ECB_QUANT_MODEL_H */
