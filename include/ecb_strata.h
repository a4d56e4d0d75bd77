/*
 * ecb_strata.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that keeps, of every read's alignments, the
 * best-scoring ones before ecb_push* sees the stream: bowtie's --best --strata, taken over the read as the tuple contract defines it.
 * Same conventions as ecb.h: plain C types, the caller owns every buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL)
 * explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_STRATA_H
#define ECB_STRATA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* set, with bit 2, in the hapflag of a record the rule dropped: one of the two bits (14, 15) that every filter of the library ignores */
#define ECB_FLAG_STRATA_DROPPED 0x4000u
#define ECB_STRATA_LOWEST 0u      /* mode: the lowest score is the best (mismatches, edit distance) */
#define ECB_STRATA_HIGHEST 1u     /* mode: the highest score is the best (an alignment score) */

/* Best stratum (ABI 4, additive).
 * In (device memory in ecb_best_strata_device, host memory in ecb_best_strata; device pointers need only 4-byte alignment -- a pointer
 * that is 16-byte aligned is read and written a vector of four records at a time, any other one record at a time):
 *   read_id   uint32 [n], hapflag uint32 [n]   as in the record tuple of ecb.h; whole reads per call, as for ecb_push_device.  The
 *             stream may begin with non-passing records that still carry the previous read's id, and the first id may be anything,
 *             0xFFFFFFFF included.  A read is a run of equal read_id; a record passes if ecb_push's filter passes its hapflag.
 *   score     int32 [n], looked at in passing records only.
 *   n         1 <= n < 2^32.     mode   ECB_STRATA_LOWEST or ECB_STRATA_HIGHEST.
 * The rule.  best(r) = the best score among the passing records of read r.  A passing record whose score is best(r) is kept -- all
 *   ties are --, every other passing record is dropped; a non-passing record is neither.
 * Out:
 *   out_hapflag   a dropped record's hapflag | 0x4 | ECB_FLAG_STRATA_DROPPED (bit 2 makes every filter reject it); any other record's
 *                 hapflag as it was.
 *   out_read_id   every record of read r that lies before r's first kept record -- dropped or non-passing -- carries r - 1 (for r = 0:
 *                 0xFFFFFFFF), so that the id still steps on a passing record only; any other record's id as it was.  The output is a
 *                 tuple stream of the same length that obeys the contract; locus, pos and the score are not written.
 *   out_counts    uint64 [4], host memory in both: {passing records, kept, dropped, reads whose first passing record was dropped}.
 *   An output may be exactly its input (out_read_id == read_id, out_hapflag == hapflag: in place); any other overlap of an output with
 *   an input or with the other output is ECB_ERR_ARG.
 * Refusals, with nothing written (no id, no flag, no count): a NULL pointer, n = 0, a mode other than 0 or 1: ECB_ERR_ARG.  n of 2^32
 * or more: ECB_ERR_LIMIT.  A read_id that falls, steps by more than 1, or steps on a non-passing record: ECB_ERR_CONTRACT, with the
 * text "strata: record R: ..." naming the lowest offender.  No index is ever derived from a read_id: a malformed stream addresses
 * nothing outside the call's buffers.
 * Two calls on the same input give the same bytes: no output depends on the order in which threads arrive. */
int ecb_best_strata_device(int device, const void* d_read_id, const void* d_hapflag, const void* d_score, uint64_t n, uint32_t mode,
                           void* d_out_read_id, void* d_out_hapflag, uint64_t* out_counts);
int ecb_best_strata(int device, const uint32_t* read_id, const uint32_t* hapflag, const int32_t* score, uint64_t n, uint32_t mode,
                    uint32_t* out_read_id, uint32_t* out_hapflag, uint64_t* out_counts);

#ifdef __cplusplus
}
#endif
#endif /* ECB_STRATA_H */
