/*
 * ecb_quant_cells_model.h -- the part of libecb.so's C ABI (include/ecb_quant.h includes this file) that runs EMASE's hierarchical models per
 * cell: ecb_quantify_cells with a gene grouping and a model, every cell a problem of its own, all cells iterated together.  Same conventions
 * as ecb.h: plain C types, the caller owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL) explains; these entry
 * points take a device ordinal.
 */
#ifndef ECB_QUANT_CELLS_MODEL_H
#define ECB_QUANT_CELLS_MODEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ecquant's models per cell (ABI 4, additive): the arguments of ecb_quantify_cells and, directly after budget_bytes, n_genes, gene (int32
 * [n_loci], gene[t] in [0, n_genes): DEVICE memory for the device entry, host memory for the host entry) and model (1, 2, 3 or 4 as
 * ecb_quantify_model numbers them).  The support does not depend on the model: n_slots is what ecb_cell_support reports.
 * Cell c's problem is ecb_quantify_cells's (ecb_quant_cells.h): its rows are the entries of column c of N with a count > 0, its unknowns its
 * support's slots x H, theta_in and scale shared tables read at the support, theta_0 = the cell's alignment counts when theta_in is NULL.
 * One step is ecb_quantify_model's (ecb_quant_model.h) applied to the cell alone, its rule included that every normalizing sum runs only
 * over the members whose own D is positive.
 * THE SUPPORT RULE: Phi_gh, Phi_g and Phi_t are sums over the cell's support only.  A member of gene g that the cell does not touch
 * contributes nothing, whatever theta_in holds there.  So cell c's step is ecb_quantify_model(sample = c) with theta_in set to 0 outside
 * the cell's support, up to rounding; with theta_in NULL the two start from the same theta_0, aln being 0 outside the support.
 * delta, W_c, the stop delta_k <= tol * W_c at each cell's own k, explained, n_iter, converged, the answers for max_iters = 0 and for a cell
 * that is not kept, has no row or has no slot, the outputs and budget_bytes: as ecb_quantify_cells.  model = 4 returns the bytes of
 * ecb_quantify_cells (gene is still checked).
 * A cell's bytes are a function of A, that cell's column of N, scale, theta_in, max_iters, tol, gene and model alone: not of which other
 * cells run, of cell_keep, of budget_bytes, of launch geometry, of scratch contents or of the entry point (no float atomics; every sum by
 * one thread in index order or by one workgroup's strided partial sums folded by a fixed tree; no sum spans two cells: a gene that two
 * cells of a batch both touch is two unrelated groups).
 * Refused with every output untouched: everything ecb_quantify_cells refuses, with its codes; a gene[t] outside [0, n_genes):
 * ECB_ERR_CONTRACT (checked on the device, also for model 4); a model outside 1..4, a null gene, n_genes = 0 with n_loci > 0: ECB_ERR_ARG;
 * a single cell whose rows hold 2^32 set haplotype bits or more (one coefficient per set bit, indexed in 32 bits; cells that share a batch
 * are planned to stay below it): ECB_ERR_LIMIT.  (cell, gene) groups x n_haps cannot overflow before n_slots x n_haps of 2^32 is refused:
 * a batch has no more groups than slots.
 * ecb_quantify_cells_model_device: the arrays in device memory;  ecb_quantify_cells_model: the same on HOST arrays. */
int ecb_quantify_cells_model_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                                    const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                    const void* d_indices_n, const void* d_data_n, const void* d_cell_keep, const void* d_scale,
                                    const void* d_theta_in, uint32_t max_iters, double tol, uint64_t budget_bytes, uint32_t n_genes,
                                    const void* d_gene, uint32_t model, uint64_t n_slots, void* d_cell_ptr, void* d_slot_locus, void* d_theta,
                                    void* d_n_iter, void* d_delta, void* d_explained, void* d_converged);
int ecb_quantify_cells_model(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                             const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                             const int32_t* indices_n, const int32_t* data_n, const uint8_t* cell_keep, const double* scale,
                             const double* theta_in, uint32_t max_iters, double tol, uint64_t budget_bytes, uint32_t n_genes, const int32_t* gene,
                             uint32_t model, uint64_t n_slots, int64_t* cell_ptr, int32_t* slot_locus, double* theta, uint32_t* n_iter,
                             double* delta, int64_t* explained, uint8_t* converged);

#ifdef __cplusplus
}
#endif

#endif /* ECB_QUANT_CELLS_MODEL_H */
