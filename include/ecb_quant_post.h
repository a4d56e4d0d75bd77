/*
 * ecb_quant_post.h -- the part of libecb.so's C ABI (include/ecb.h, through ecb_quant.h, which includes this file) that returns what the EM
 * exists to compute: the posterior probability of every alignment of every equivalence class at a given theta.  Same conventions as ecb.h:
 * plain C types, the caller owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL) explains; these entry points take a
 * device ordinal, not a handle.
 */
#ifndef ECB_QUANT_POST_H
#define ECB_QUANT_POST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ecquant's posterior (ABI 4, additive): one probability per set bit of A -- what the reference's multiply(axis=2) and normalize_reads leave
 * in the matrix before sum(axis=READ) (AlignmentPropertyMatrix.py:219-384), and what AlignmentPropertyMatrix.save(incidence_only=False) stores.
 * A (n_ecs, n_loci, n_haps, nnz_a, indptr, indices, data = haplotype bitmasks), scale (NULL: 1 everywhere), n_genes, gene and model: as
 * ecb_quantify_model takes them; theta: float64 [n_haps x n_loci] row-major, required.  Model 4, the flat model, ignores the grouping: gene may
 * then be NULL, and is still checked when it is given.  There is no N: the posterior of a row does not depend on its count, and a row of
 * weight 0 gets its posterior like any other.  n_bits: the set bits of A, as ecb_csr_to_hapcsc reports them with csc_indices = NULL.
 * With phi = theta * scale:
 *   model 4:     p[e, t, h] = phi[h, t] / d[e], d[e] as ecb_quantify defines it; all of row e is 0 when d[e] = 0
 *   models 1-3:  the product of factors ecb_quantify_model defines (every normalizing sum over the members whose own D is positive); a row
 *                with D(S(e)) = 0 is all 0
 * so that the sum over rows of w[e] p[e, t, h] is the theta' of one step of ecb_quantify / ecb_quantify_model from the same theta.
 * Outputs:
 *   post      float64 [n_bits], in BIT ORDER: the non-zeros in A's storage order, the set bits of one non-zero lowest first (a stored mask
 *             of 0 has no bits and no values)
 *   bit_ptr   int64 [nnz_a + 1] or NULL: the exclusive scan of the popcounts -- non-zero i owns post[bit_ptr[i] .. bit_ptr[i + 1]),
 *             bit_ptr[nnz_a] = n_bits
 *   row_mass  float64 [n_ecs] or NULL: d[e] (for models 1-3: D(S(e)), the same sum) -- 0 marks the rows nothing explains
 * The result is a function of the inputs alone: no float atomics, every sum in a fixed order.
 * Refused with every output untouched: what ecb_quantify_model refuses on A, scale, gene and model, with its codes; an entry of theta that
 * is NaN, infinite or negative: ECB_ERR_CONTRACT; a null theta, a null post with n_bits > 0, an n_bits other than A's: ECB_ERR_ARG; 2^32 set
 * bits or more: ECB_ERR_LIMIT.  n_ecs = 0 or nnz_a = 0 is no error: nothing is written but bit_ptr.
 * ecb_posterior_device: the arrays in device memory;  ecb_posterior: the same on HOST arrays. */
int ecb_posterior_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                         const void* d_indices_a, const void* d_data_a, const void* d_scale, const void* d_theta, uint32_t n_genes,
                         const void* d_gene, uint32_t model, uint64_t n_bits, void* d_post, void* d_bit_ptr, void* d_row_mass);
int ecb_posterior(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                  const int32_t* indices_a, const int32_t* data_a, const double* scale, const double* theta, uint32_t n_genes,
                  const int32_t* gene, uint32_t model, uint64_t n_bits, double* post, int64_t* bit_ptr, double* row_mass);

/* CSR -> per-haplotype CSC with a payload (ABI 4, additive; the conversion itself: ecb.h, f-2): ecb_csr_to_hapcsc* with one more input --
 * values: float64, one per set bit of A in BIT ORDER (the non-zeros in storage order, the set bits of one lowest first: ecb_posterior's post) -- and one more output -- csc_data:
 * float64, laid out like csc_indices, so csc_data[k] is the value of the (row, column, haplotype) csc_indices[k] names.  csc_indptr and
 * csc_indices come out byte for byte as ecb_csr_to_hapcsc* writes them; the values are moved, never recomputed.  csc_indices, csc_data or
 * csc_indptr = NULL: *total alone, as there.  Refusals: ecb_csr_to_hapcsc*'s; a null values with set bits to move: ECB_ERR_ARG.
 * The host entry point's `capacity` is the room of csc_indices and of csc_data alike. */
int ecb_csr_to_hapcsc_values_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, const void* d_indptr_a,
                                    const void* d_indices_a, const void* d_data_a, const void* d_values, void* d_csc_indptr,
                                    void* d_csc_indices, void* d_csc_data, uint64_t* total);
int ecb_csr_to_hapcsc_values(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, const int32_t* indptr_a, const int32_t* indices_a,
                             const int32_t* data_a, const double* values, int32_t* csc_indptr, int32_t* csc_indices, double* csc_data,
                             uint64_t capacity, uint64_t* total);

#ifdef __cplusplus
}
#endif
#endif /* ECB_QUANT_POST_H */
