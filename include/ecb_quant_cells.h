/*
 * ecb_quant_cells.h -- the part of libecb.so's C ABI (include/ecb_quant.h includes this file) that estimates abundances per cell: one EM for
 * every column of a multisample N, all cells iterated together, the result sparse.  Same conventions as ecb.h: plain C types, the caller
 * owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL) explains; these entry points take a device ordinal.
 */
#ifndef ECB_QUANT_CELLS_H
#define ECB_QUANT_CELLS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ecquant per cell (ABI 4, additive).  A: CSR over (EC, locus), values = haplotype bitmasks; N: CSC over (EC, sample) -- as ecb_quantify
 * takes them; there is no `sample`.  cell_keep: uint8 [n_samples] or NULL -- non-zero = quantify this cell, NULL = every cell (ecselect's
 * sample_keep convention).  scale, theta_in: float64 [n_haps x n_loci] row-major, either may be NULL; theta_in is ONE table shared by every
 * cell (a pooled estimate to start from), read at the cell's support.
 * The problem of cell c: its rows are the entries k of column c of N with a count n_k > 0, each with the pattern of row e_k of A (an EC listed
 * twice in a column is two rows: the same as one row of the summed count, up to rounding).  support(c) = the loci t at which some row of
 * the cell holds a non-zero (e_k, t) with a mask other than 0, ascending; one SLOT per locus of a support.  With theta_in NULL, theta_0 on the
 * support = the cell's alignment counts (exact integers: aln of ecb_count_alignments(sample = c); every slot then has an entry > 0).  A step,
 * delta_k, W (here W_c, over the cell's rows that hold a set bit), the stop delta_k <= tol * W_c, `explained` and a row with d = 0 reading as
 * r = 0 are ecb_quantify's definitions applied to the cell alone; each cell stops at its own k.  max_iters = 0 returns theta_0 and, no step
 * having been asked of any cell, n_iter = 0, delta = 0, explained = 0 and converged = 1 for every cell (ecb_quantify reports 0 there).  A
 * cell that is not kept, has no row or has an empty support: no slots, n_iter 0, delta 0, explained 0, converged 1.
 * Outputs, in cell order: cell_ptr int64 [n_samples + 1] (cell c owns slots [cell_ptr[c], cell_ptr[c + 1])); slot_locus int32 [n_slots];
 * theta float64 [n_slots x n_haps], the H values of a slot together (a slot where theta_in is 0 is still written, as 0); per cell, each may
 * be NULL: n_iter uint32 [S], delta float64 [S], explained int64 [S], converged uint8 [S] -- DEVICE arrays for the device entry, host arrays
 * for the host entry.
 * budget_bytes: the cells are run in batches, in cell order, whose working set aims at this many bytes of device memory; 0 = half of what is
 * free.  A target, not a limit: a cell that alone exceeds it runs alone.
 * A cell's bytes are a function of A, that cell's column of N, scale, theta_in, max_iters and tol alone: not of which other cells run, of
 * cell_keep, of budget_bytes, of launch geometry, of scratch contents or of the entry point (no float atomics; every sum by one thread in
 * index order or by one workgroup's strided partial sums folded by a fixed tree; W_c and explained are exact integers).
 *
 * ecb_cell_support: cell_ptr alone -- the targets detected per cell -- and slot_locus when that is non-NULL and slot_capacity >= the number
 * of slots, which *n_slots (HOST, may be NULL) receives either way.  ecb_quantify_cells takes n_slots as the caller learned it there.
 * Refused with every output untouched: what ecb_quantify refuses, with its codes (but n_samples = 0, which is no error here: cell_ptr = {0});
 * a support of another size than n_slots: ECB_ERR_ARG, the text names both; a null cell_ptr, or with n_slots > 0 a null slot_locus or
 * theta: ECB_ERR_ARG; a support of 2^31 slots or n_slots x n_haps of 2^32 or more, or a single cell that expands to 2^30 non-zeros:
 * ECB_ERR_LIMIT.
 * *_device: the arrays in device memory; the others: the same on HOST arrays (the library allocates and frees its own device buffers). */
int ecb_cell_support_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                            const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                            const void* d_indices_n, const void* d_data_n, const void* d_cell_keep, void* d_cell_ptr, void* d_slot_locus,
                            uint64_t slot_capacity, uint64_t* n_slots);
int ecb_cell_support(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                     const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                     const int32_t* indices_n, const int32_t* data_n, const uint8_t* cell_keep, int64_t* cell_ptr, int32_t* slot_locus,
                     uint64_t slot_capacity, uint64_t* n_slots);
int ecb_quantify_cells_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                              const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                              const void* d_indices_n, const void* d_data_n, const void* d_cell_keep, const void* d_scale, const void* d_theta_in,
                              uint32_t max_iters, double tol, uint64_t budget_bytes, uint64_t n_slots, void* d_cell_ptr, void* d_slot_locus,
                              void* d_theta, void* d_n_iter, void* d_delta, void* d_explained, void* d_converged);
int ecb_quantify_cells(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                       const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                       const int32_t* indices_n, const int32_t* data_n, const uint8_t* cell_keep, const double* scale, const double* theta_in,
                       uint32_t max_iters, double tol, uint64_t budget_bytes, uint64_t n_slots, int64_t* cell_ptr, int32_t* slot_locus,
                       double* theta, uint32_t* n_iter, double* delta, int64_t* explained, uint8_t* converged);

#ifdef __cplusplus
}
#endif

#endif /* ECB_QUANT_CELLS_H */
