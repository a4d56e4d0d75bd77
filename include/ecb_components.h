/*
 * ecb_components.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that groups a .bin's targets by the reads they
 * share.  Same conventions as ecb.h: plain C types, the caller owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL)
 * explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_COMPONENTS_H
#define ECB_COMPONENTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ecclusters (ABI 4, additive): the connected components of the target-EC incidence of a .bin -- the transitive closure of the pairwise
 * "shares multireads with" relation, and the decomposition under which the EM is separable.
 * A: CSR over (EC, locus), values = haplotype bitmasks; N: CSC over (EC, sample) as the .bin stores it.
 * w[e] is count-alignments' weight (ecb_count.h): the sum of row e of N over all samples (sample = -1) or its entry in one column
 * (0 <= sample < n_samples); an EC that N does not list weighs 0, one listed twice in a column has its counts added.
 * The MEMBERS of row e are its columns whose mask is not 0 (a mask of 0 is no alignment, as in ecb_count.h).
 * Row e LINKS when w[e] >= min_count and it has at least one member.  With min_count = 0 every row with a member links (N is still checked).
 * The COMPONENTS are the connected components of the graph on the n_loci loci in which the members of every linking row are joined; a locus
 * that no linking row holds is a component of its own.  They are numbered 0 .. C-1 in ascending order of their smallest locus: the result
 * is a function of the input alone, comp_of_locus[0] == 0 and comp_of_locus[t] <= t.
 * Outputs (T = n_loci, E = n_ecs; any may be NULL except comp_of_locus and out_sizes):
 *   comp_of_locus  int32 [T]  the component of each locus
 *   comp_of_ec     int32 [E]  the component of a linking row's members, -1 for a row that does not link
 *   comp_loci      int32 [T]  per component, its number of loci; all T entries written, 0 at and beyond C
 *   comp_ecs       int32 [T]  per component, its number of linking rows; all T entries written, 0 at and beyond C
 *   comp_reads     int64 [T]  per component, the sum of w[e] over its linking rows; all T entries written, 0 at and beyond C
 *   out_sizes      uint64 [4] (host memory in both entry points) {C, linking rows, loci of the largest component, components with two
 *                             loci or more}
 * All sums are exact integers (no float atomics), the same whatever the order of arrival; two calls give the same bytes.
 * Refusals: what ecb_count_alignments refuses, with its codes (ECB_ERR_ARG, ECB_ERR_LIMIT -- nnz_a of 2^30 or more among them --, a sample
 * outside [-1, n_samples): ECB_ERR_CONTRACT); min_count < 0, a NULL comp_of_locus or out_sizes: ECB_ERR_ARG.  A malformed A or N (the
 * contract of ecb_count.h) is ECB_ERR_CONTRACT and nothing is written.
 * ecb_components_device: device pointers;  ecb_components: the same on HOST arrays (the library allocates and frees its own device
 * buffers). */
int ecb_components_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                          const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                          const void* d_indices_n, const void* d_data_n, int64_t sample, int64_t min_count, void* d_comp_of_locus,
                          void* d_comp_of_ec, void* d_comp_loci, void* d_comp_ecs, void* d_comp_reads, uint64_t* out_sizes);
int ecb_components(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                   const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                   const int32_t* indices_n, const int32_t* data_n, int64_t sample, int64_t min_count, int32_t* comp_of_locus,
                   int32_t* comp_of_ec, int32_t* comp_loci, int32_t* comp_ecs, int64_t* comp_reads, uint64_t* out_sizes);

#ifdef __cplusplus
}
#endif
#endif /* ECB_COMPONENTS_H */
