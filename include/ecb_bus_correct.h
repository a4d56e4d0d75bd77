/*
 * ecb_bus_correct.h -- the part of libecb.so's C ABI (include/ecb.h, which includes this file) that snaps the barcodes of a kallisto BUS
 * file's records onto a whitelist before ecb_bus_molecules sees them.  Same conventions as ecb.h: plain C types, the caller owns every
 * buffer, 0 = OK, < 0 = an ECB_ERR_* code that ecb_last_error(NULL) explains; these entry points take a device ordinal, not a handle.
 */
#ifndef ECB_BUS_CORRECT_H
#define ECB_BUS_CORRECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the status of a record (out_status, and the order of out_sizes) */
#define ECB_BUS_EXACT 0u          /* the barcode is in the whitelist: kept as it is */
#define ECB_BUS_CORRECTED 1u      /* not in it, and exactly one whitelist barcode differs in exactly one base: kept, the barcode replaced */
#define ECB_BUS_NO_CANDIDATE 2u   /* not in it, no whitelist barcode one base away: dropped */
#define ECB_BUS_AMBIGUOUS 3u      /* not in it, two or more whitelist barcodes one base away: dropped */

/* Barcode correction (ABI 4, additive): bustools correct's rule ("bus2ec"), on the records as they lie in the file.
 * In:
 *   records      as in ecb_bus_molecules: n x 32 bytes, little endian, any alignment; the barcode is the first uint64.  1 <= n < 2^30.
 *   bclen        bases per barcode, 1 .. 32, 2 bits per base.
 *   whitelist    uint64 [n_white], strictly ascending, every value below 4^bclen.  1 <= n_white < 2^31.
 * The rule.  A base is 2 bits and differs if either bit does.  A record whose barcode is in the whitelist is ECB_BUS_EXACT, whatever
 *   its neighbours.  Otherwise its 3 x bclen single-base neighbours -- they are distinct -- are looked up: exactly one of them in the
 *   whitelist: ECB_BUS_CORRECTED, the barcode becomes that one; none: ECB_BUS_NO_CANDIDATE; two or more: ECB_BUS_AMBIGUOUS.
 * Out (device memory in ecb_bus_correct_device, host memory in ecb_bus_correct; out_sizes is host memory in both):
 *   out_records  the exact and the corrected records, in the file's order, 32 bytes each, any alignment: the barcode of a corrected
 *                record replaced, the other 24 bytes (UMI, ec, count, flags, pad) as they were.  Room for cap_out records.  It may not
 *                overlap records: ECB_ERR_ARG.
 *   out_status   uint8 [n], the status of every input record; may be NULL.
 *   out_sizes    uint64 [4]  {exact, corrected, without a candidate, ambiguous}.  Records out = the first two added.
 * Capacity: the bound from the input alone is that the records kept are at most n.  A cap_out smaller than the records kept is
 * ECB_ERR_ARG; every size is known before the first output byte is written.
 * Refusals: a NULL or zero argument (out_status aside), bclen outside 1 .. 32: ECB_ERR_ARG.  n of 2^30 or more, n_white of 2^31 or more:
 * ECB_ERR_LIMIT.  Malformed input is ECB_ERR_CONTRACT, naming the lowest offender: "bus: whitelist entry J: ..." (not above the entry
 * before it, or a bit at or above 2 x bclen; looked at first), "bus: record R: a barcode bit at or above 2 x bclen".  A refusal writes
 * nothing: no output record, no status, no size.
 * Two calls on the same input give the same bytes: no output depends on the order in which threads arrive. */
int ecb_bus_correct_device(int device, const void* d_records, uint64_t n, uint32_t bclen, const void* d_whitelist, uint64_t n_white, uint64_t cap_out,
                           void* d_out_records, void* d_out_status, uint64_t* out_sizes);
int ecb_bus_correct(int device, const void* records, uint64_t n, uint32_t bclen, const uint64_t* whitelist, uint64_t n_white, uint64_t cap_out,
                    void* out_records, uint8_t* out_status, uint64_t* out_sizes);

#ifdef __cplusplus
}
#endif
#endif /* ECB_BUS_CORRECT_H */
