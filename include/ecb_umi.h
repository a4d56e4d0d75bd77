/*
 * ecb_umi.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that makes the reads of one molecule one read
 * before ecb_push* sees the stream: bus2ec's UMI rule (include/ecb_bus.h), stated on tuple streams.
 * Same conventions as ecb.h: plain C types, the caller owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL)
 * explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_UMI_H
#define ECB_UMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* a molecule key that joins nothing: a read that carries it is a molecule of its own */
#define ECB_UMI_NONE 0xFFFFFFFFFFFFFFFFull

/* Collapse UMIs (ABI 4, additive).
 * In (device memory in ecb_collapse_umis_device, host memory in ecb_collapse_umis; a pointer is aligned to its element: 4 bytes, 8 for
 * mol_key):
 *   read_id, locus, hapflag   uint32 [n], as in the record tuple of ecb.h; whole reads per call.  The first id may be anything.  A record
 *             passes if ecb_push's filter passes its hapflag; its haplotype is hapflag >> ECB_HAP_SHIFT.  A read is a run of equal
 *             read_id, and the contract makes every read begin with a passing record: the reads of the stream are numbered 0, 1, 2, ...
 *             from the first id that a passing record carries.  Non-passing records in front of the stream that carry the id before
 *             that one (0xFFFFFFFF before read 0) belong to no read.  A stream without a passing record holds no read.
 *   mol_key   uint64 [n_reads]: read r's molecule.  Reads with equal keys are one molecule; ECB_UMI_NONE never joins.
 *   n         1 <= n < 2^30.    n_reads   the number of reads in the stream.    n_loci, n_haps   as in ecb_config; n_haps <= 31.
 * The rule.  A read's target set is the set of distinct (locus, haplotype) of its passing records.
 *   A molecule of one read stays that read: its passing records as they are, in stream order, duplicates included.
 *   A molecule of k > 1 reads becomes one read whose target set is the intersection of the k sets (a target one read names twice counts
 *   once for that read): discarded if that is empty, otherwise one record per target in ascending (locus, haplotype) order with
 *   hapflag = haplotype << ECB_HAP_SHIFT and every flag bit zero.  Non-passing records are not emitted.
 *   The surviving molecules are numbered 0, 1, 2, ... in the order of their first (lowest) read.
 * Out (device / host memory as the inputs):
 *   out_read_id, out_locus, out_hapflag   uint32, capacity n: a tuple stream that obeys the contract, ids from 0; out_counts[4] records.
 *   out_first_read   uint32, capacity n_reads: molecule m's first read, 0-based within the call; out_counts[1] - out_counts[3] entries.
 *   out_counts       uint64 [6], host memory in both: {reads in, molecules, molecules of k > 1, molecules discarded, records out, reads
 *                    whose key is ECB_UMI_NONE}.
 * Refusals, with nothing written (no record, no first read, no count): a NULL pointer, n = 0, n_haps outside 1 .. 31, n_loci outside
 * 1 .. 2^26 - 3, a misaligned pointer, an output that shares a byte with an input or with another output: ECB_ERR_ARG.  n of 2^30 or
 * more (the sort's bound): ECB_ERR_LIMIT.  ECB_ERR_CONTRACT, with the text "umi: record R: ..." naming the lowest offender: a read_id that
 * falls, steps by more than 1, or steps on a non-passing record; a passing record whose locus is n_loci or more or whose haplotype is
 * n_haps or more; and, on a stream that is otherwise sound, an n_reads that is not the stream's number of reads -- R is then the record
 * at which read n_reads begins, or n - 1 where the stream ends before read n_reads - 1.  No index is ever derived from unvalidated input.
 * Two calls on the same input give the same bytes: nothing is placed by the order in which threads arrive. */
int ecb_collapse_umis_device(int device, const void* d_read_id, const void* d_locus, const void* d_hapflag, const void* d_mol_key, uint64_t n,
                             uint64_t n_reads, uint32_t n_loci, uint32_t n_haps, void* d_out_read_id, void* d_out_locus, void* d_out_hapflag,
                             void* d_out_first_read, uint64_t* out_counts);
int ecb_collapse_umis(int device, const uint32_t* read_id, const uint32_t* locus, const uint32_t* hapflag, const uint64_t* mol_key, uint64_t n,
                      uint64_t n_reads, uint32_t n_loci, uint32_t n_haps, uint32_t* out_read_id, uint32_t* out_locus, uint32_t* out_hapflag,
                      uint32_t* out_first_read, uint64_t* out_counts);

#ifdef __cplusplus
}
#endif
#endif /* ECB_UMI_H */
