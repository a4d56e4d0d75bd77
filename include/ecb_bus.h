/*
 * ecb_bus.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that turns the records of a kallisto BUS file into
 * the rows and the cell counts of a multisample .bin.  Same conventions as ecb.h: plain C types, the caller owns every buffer, 0 = OK,
 * < 0 = an ECB_ERR_* code that ecb_last_error(NULL) explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_BUS_H
#define ECB_BUS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECB_BUS_NO_UMI 1u        /* flags bit 0: every record is `count` reads of its EC in its cell; the UMI is ignored */
#define ECB_BUS_MAX_UMILEN 16u   /* UMI mode: the UMI shares a 64-bit sort key with the cell's rank, 2 x 16 bits of it */

/* bus2ec (ABI 4, additive): bustools count's rule for EC matrices ("bus2ec"), on the records as they lie in the file.
 * In:
 *   records      n x 32 bytes, little endian, any alignment: uint64 barcode; uint64 umi; int32 ec; uint32 count; uint32 flags; uint32 pad
 *                (flags and pad are ignored); in any order, repeats allowed.  1 <= n < 2^30.
 *   bclen, umilen  bases per barcode / UMI, 1 .. 32, 2 bits per base; umilen above ECB_BUS_MAX_UMILEN is ECB_ERR_LIMIT unless
 *                ECB_BUS_NO_UMI is set.
 *   ec_ptr, ec_targets  matrix.ec as a CSR over target ids: uint32 ec_ptr[n_ecs + 1] from 0 to n_ec_targets, never falling; the ids of a
 *                line strictly ascending and below n_targets.  n_ecs < 2^31.
 *   target_col, target_hap  uint32 [n_targets]: the column (below n_loci) and haplotype (below n_haps <= 31) of every target; two
 *                targets may share both as long as no row holds the two (a row that does is refused: a mask is the sum of 2^h).
 *   keep, n_keep the barcodes to keep, uint64, strictly ascending; NULL: all.
 * The rule.  A record counts when its barcode is kept.  The CELLS are the distinct barcodes of the records that count, ascending.
 *   UMI mode: a molecule is a distinct (barcode, UMI) -- `count` is ignored --, naming the distinct ECs e_1 .. e_k.  k = 1: one read of line
 *   e_1.  k > 1: its target set is the intersection of the lines e_1 .. e_k; empty: the molecule is discarded, otherwise it is one read of
 *   a NEW row with that set.
 *   ECB_BUS_NO_UMI: a record is `count` reads of line ec (a count of 0: no read); no intersection is taken.
 * Out (device memory in ecb_bus_molecules_device, host memory in ecb_bus_molecules; out_sizes is host memory in both):
 *   out_barcodes uint64 [cells]       the cells
 *   CSR A        out_indptr_a int32 [rows + 1], out_indices_a / out_data_a int32 [nnz_a]: first the matrix.ec lines that received a read,
 *                ascending, then one row per surviving k > 1 molecule in ascending (barcode, UMI) order; per row the columns ascending,
 *                the mask of a column the OR of 1 << haplotype over the row's targets there -- ecb_combine's contract for a part
 *   CSC N        out_indptr_n int32 [cells + 1], out_indices_n / out_data_n int32 [nnz_n]: per cell its rows ascending, reads summed
 *   out_row_line int32 [rows]         the matrix.ec line a row came from, -1 for a new row
 *   out_sizes    uint64 [8]           {cells, rows, nnz_a, nnz_n, molecules (no-UMI: records of a kept barcode with a count above 0),
 *                                     molecules of k > 1, molecules discarded, new rows}
 * Capacities: the room of out_barcodes (cap_cells; out_indptr_n holds cap_cells + 1), of out_row_line (cap_rows; out_indptr_a holds
 * cap_rows + 1), of A's and of N's non-zeros.  Bounds from the input alone: cells, rows and nnz_n are at most n; nnz_a is at most the sum
 * over the records of the length of their EC's line.  A capacity too small is ECB_ERR_ARG, and nothing is written.
 * Refusals: a NULL or zero argument, n_haps > 31, bclen or umilen outside 1 .. 32: ECB_ERR_ARG.  n of 2^30 or more, 2^30 (row, target)
 * pairs or more, a count of N beyond int32, umilen beyond ECB_BUS_MAX_UMILEN: ECB_ERR_LIMIT.  Malformed input is ECB_ERR_CONTRACT with
 * nothing written: "bus: matrix.ec line L: ..." for the lowest offending line (pointers, a target id at or beyond n_targets, ids not
 * strictly ascending), "bus: record R: ..." for the lowest offending record (ec below 0 or at or beyond n_ecs, a barcode bit at or above
 * 2 bclen, a UMI bit at or above 2 umilen), a target map beyond n_loci / n_haps, two targets of one row in one (column, haplotype), a keep
 * list that is not strictly ascending.
 * Two calls on the same input give the same bytes: no output depends on the order in which threads arrive. */
int ecb_bus_molecules_device(int device, const void* d_records, uint64_t n, uint32_t bclen, uint32_t umilen, uint32_t flags, uint32_t n_ecs,
                             uint64_t n_ec_targets, const void* d_ec_ptr, const void* d_ec_targets, uint32_t n_targets, const void* d_target_col,
                             const void* d_target_hap, uint32_t n_loci, uint32_t n_haps, const void* d_keep, uint64_t n_keep, uint64_t cap_cells,
                             uint64_t cap_rows, uint64_t cap_a, uint64_t cap_n, void* d_out_barcodes, void* d_out_indptr_a, void* d_out_indices_a,
                             void* d_out_data_a, void* d_out_indptr_n, void* d_out_indices_n, void* d_out_data_n, void* d_out_row_line,
                             uint64_t* out_sizes);
int ecb_bus_molecules(int device, const void* records, uint64_t n, uint32_t bclen, uint32_t umilen, uint32_t flags, uint32_t n_ecs,
                      uint64_t n_ec_targets, const uint32_t* ec_ptr, const uint32_t* ec_targets, uint32_t n_targets, const uint32_t* target_col,
                      const uint32_t* target_hap, uint32_t n_loci, uint32_t n_haps, const uint64_t* keep, uint64_t n_keep, uint64_t cap_cells,
                      uint64_t cap_rows, uint64_t cap_a, uint64_t cap_n, uint64_t* out_barcodes, int32_t* out_indptr_a, int32_t* out_indices_a,
                      int32_t* out_data_a, int32_t* out_indptr_n, int32_t* out_indices_n, int32_t* out_data_n, int32_t* out_row_line,
                      uint64_t* out_sizes);

#ifdef __cplusplus
}
#endif
#endif /* ECB_BUS_H */
